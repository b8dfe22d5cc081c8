"""CPU: the export operators (inverserenderingofindoorscene_amd/export.py) without a GPU -- the numpy checker against the fixtures made from the
reference's own statements (tests/golden/g26_export_*.npz), the resize's index rule and the mosaic geometry enumerated, the input condition of
the byte bound on every input set the GPU tests use, the Meta kernels' shapes, every refusal (wrapper, operators, C ABI), and the kernels'
decisions (csrc/sgr_export.h) compiled for the host as a stand-alone program under -fsanitize=address,undefined, against the fixtures."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import export_checker as K
from conftest import GOLDEN_DIR, ROOT
import inverserenderingofindoorscene_amd as sgr
from inverserenderingofindoorscene_amd import _lib

IMAGE_CASES = ("tiny", "row", "odd", "down", "same")
BLOCK_KINDS = ("albedo", "normal", "rough", "depth", "rendered", "shading")


def fixture(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g26_export_{name}.npz"))


def fixture_sets(name):
    """(kind, key suffix, x, size, scale) of an image fixture"""
    z = fixture(name)
    size = tuple(int(v) for v in z["size"])
    for kind in BLOCK_KINDS:
        yield z, kind, kind, z["x_" + kind], (size if kind in K.RESIZED else None), (z["scale"] if kind == "albedo" and "scale" in z.files else None)
    if name == "same":
        for C in (1, 3):
            for kind in ("image", "image_gamma"):
                yield z, kind, f"{kind}{C}", z[f"x_image{C}"], None, None


def close12(a, b):
    """the fixture's t is the value the reference casts: for the albedo that is np.clip(255 a, 0, 255), so both sides are clipped alike"""
    a, b = np.clip(a, 0, 255), np.clip(b, 0, 255)
    return np.abs(a - b).max() <= 1e-12 * max(1.0, float(np.abs(b).max()))


def t64_of(x, kind, size, scale):
    """the checker's fp64 t, which test_checker_reproduces_the_reference_fixtures pins to the fixture's: unclipped, so that a saturated
    value sits beyond the clip and is not taken for one near an integer"""
    return K.image_t(x, kind, size, scale, dtype=np.float64, clip=False)


@pytest.mark.parametrize("name", IMAGE_CASES)
def test_checker_reproduces_the_reference_fixtures(name):
    for z, kind, key, x, size, scale in fixture_sets(name):
        assert "not executed from the reference's own dependency" in str(z["notes"])
        t64 = K.image_t(x, kind, size, scale, dtype=np.float64)
        t32 = K.image_t(x, kind, size, scale, dtype=np.float32)
        assert t64.shape == z["t64_" + key].shape and close12(t64, z["t64_" + key]), (name, key)
        assert t32.dtype == np.float32 and np.array_equal(K.quantise(t32), z["ref_" + key]), (name, key)
        e_t = float(np.abs(np.clip(t32.astype(np.float64), 0, 255) - np.clip(t64, 0, 255)).max())
        assert e_t == pytest.approx(float(z["e_t_" + key]), rel=1e-6, abs=1e-12) and e_t < 2.5e-4, (name, key, e_t)
        assert np.array_equal(K.image_t(x, kind, size, scale, bgr=True, dtype=np.float64), t64[..., ::-1])


def test_checker_reproduces_the_env_fixture():
    z = fixture("env")
    assert "not executed from the reference's own dependency" in str(z["notes"]) and "fp32 array whatever it is given" in str(z["notes"])
    for tag in ("a", "b"):
        env, (nrows, ncols, gap) = z["env_" + tag], (int(v) for v in z["cfg_" + tag])
        t32 = K.env_mosaic_t(env, nrows, ncols, gap, dtype=np.float32)
        assert np.array_equal(K.quantise(t32), z["ref_mosaic_" + tag]), tag
        assert close12(K.env_mosaic_t(env, nrows, ncols, gap, dtype=np.float64), z["t64_mosaic_" + tag])
        assert np.array_equal(K.env_hwc(env, True), z["ref_hwc_" + tag]) and z["ref_hwc_" + tag].dtype == np.float32
    assert z["ref_mosaic_a"].shape == (2, 4 * 9 + 1, 5 * 17 + 1, 3)      # R = 7, nrows = 3: four rows of tiles; C = 9, ncols = 4: five columns


def test_fixture_cases_cover_what_they_are_for():
    z = fixture("odd")
    assert z["x_albedo"].shape == (3, 3, 6, 10) and tuple(z["size"]) == (9, 13) and len(set(z["scale"].tolist())) == 3
    assert len({float(z["x_depth"][b].mean()) for b in range(3)}) == 3 and len({float(z["x_rendered"][b].max()) for b in range(3)}) == 3
    assert (z["ref_albedo"] == 255).any() and (t64_of(z["x_albedo"], "albedo", (9, 13), z["scale"]) > 255 + 1e-3).any()      # saturation, well beyond the clip
    assert fixture("tiny")["x_albedo"].shape == (1, 3, 1, 1) and fixture("tiny")["ref_albedo"].shape == (1, 3, 2, 3)
    assert fixture("row")["x_rough"].shape == (1, 1, 1, 7) and fixture("row")["ref_rough"].shape == (1, 2, 11, 1)
    assert fixture("down")["x_normal"].shape[2:] == (9, 13) and fixture("down")["ref_normal"].shape[1:3] == (6, 10)
    assert not bool(fixture("same")["resized"]) and fixture("same")["ref_image1"].shape == (2, 5, 7, 3)


# ---- the input condition of the byte bound --------------------------------------------------------------------------------------------------

def test_input_condition_on_the_fixtures():
    for name in IMAGE_CASES:
        for z, kind, key, x, size, scale in fixture_sets(name):
            K.check_bytes(z["ref_" + key], t64_of(x, kind, size, scale), float(z["e_t_" + key]), f"{name} {key}: the reference's fp32 bytes")
    z = fixture("env")
    for tag in ("a", "b"):
        env, (nrows, ncols, gap) = z["env_" + tag], (int(v) for v in z["cfg_" + tag])
        K.check_bytes(z["ref_mosaic_" + tag], K.env_mosaic_t(env, nrows, ncols, gap, clip=False), float(z["e_t_mosaic_" + tag]), f"env mosaic {tag}: the reference's fp32 bytes")


def test_input_condition_on_every_set_the_gpu_tests_use():
    worst = 0.0
    for tag, kind, x, size, scale in K.gpu_input_sets():
        e_t = K.input_condition(K.image_t(x, kind, size, scale, dtype=np.float32, clip=False), K.image_t(x, kind, size, scale, dtype=np.float64, clip=False), tag)
        worst = max(worst, e_t)
    for tag, env, nrows, ncols, gap in K.gpu_env_sets():
        worst = max(worst, K.input_condition(K.env_mosaic_t(env, nrows, ncols, gap, dtype=np.float32, clip=False), K.env_mosaic_t(env, nrows, ncols, gap, dtype=np.float64, clip=False), tag))
    assert worst < 2.5e-4, worst      # 4 e_t stays below the floor of 1e-3: delta is 1e-3 throughout


# ---- the index rule and the mosaic geometry, enumerated ---------------------------------------------------------------------------------

def dense_src(d, n_in, n_out):
    """the rule as the issue states it, one index at a time"""
    f = np.float32((d + 0.5) * (float(n_in) / float(n_out)) - 0.5)
    s = int(np.floor(f))
    f = np.float32(f - np.float32(s))
    if s < 0:
        s, f = 0, np.float32(0)
    if s >= n_in - 1:
        s, f = n_in - 1, np.float32(0)
    return s, f


def test_index_rule_enumerated():
    for n_in in range(1, 13):
        for n_out in range(1, 13):
            s, f = K.src_of(n_in, n_out)
            assert f.dtype == np.float32
            for d in range(n_out):
                ws, wf = dense_src(d, n_in, n_out)
                assert (int(s[d]), f[d]) == (ws, wf), (n_in, n_out, d)
                assert 0 <= s[d] <= n_in - 1 and 0 <= f[d] < 1 and (s[d] < n_in - 1 or f[d] == 0)
            assert np.all(np.diff(s) >= 0)
            if n_in == n_out:
                assert np.array_equal(s, np.arange(n_in)) and not f.any()      # the same size: the identity
    x = np.random.default_rng(1).random((2, 5, 7)).astype(np.float32)
    assert np.array_equal(K.resize_linear(x, 5, 7), x)
    # not torch's rule: the scale formed in fp32 moves the coordinate (sgr_regress.h: src_index stays as it is)
    s, f = K.src_of(41, 60)
    r = np.maximum(np.float32(41 / 60) * (np.arange(60, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), 0)
    assert np.any(f != (r - np.floor(r)).astype(np.float32))


def test_mosaic_geometry_enumerated():
    for R in range(1, 13):
        for nrows in range(1, R + 1):
            for eh, gap in ((8, 1), (3, 0), (1, 2)):
                iy, _, ty, _, Hm, _ = K.mosaic_geometry(R, R, eh, eh, nrows, nrows, gap)
                assert iy == int(R / nrows) and ty == len(np.arange(0, R, iy)) and Hm == ty * (eh + gap) + gap      # utils.py:107-113
                assert (ty - 1) * iy < R and ty >= nrows
    assert K.mosaic_geometry(7, 9, 8, 16, 3, 4)[2:4] == (4, 5)


# ---- Meta kernels -------------------------------------------------------------------------------------------------------------------------

def m(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def test_meta_shapes_and_dtypes():
    B, h, w = 3, 6, 10
    for kind, C in (("albedo", 3), ("normal", 3), ("rough", 1), ("depth", 1), ("rendered", 3)):
        out = sgr.export_image(m(B, C, h, w), kind, size=(9, 13), bgr=True)
        assert tuple(out.shape) == (B, 9, 13, C) and out.dtype == torch.uint8
        assert tuple(sgr.export_image(m(B, C, h, w), kind).shape) == (B, h, w, C)
    assert tuple(sgr.export_image(m(B, 3, h, w), "albedo", (2, 2), scale=m(B)).shape) == (B, 2, 2, 3)
    for kind in ("shading", "image", "image_gamma"):
        assert tuple(sgr.export_image(m(B, 3, h, w), kind).shape) == (B, h, w, 3)
        assert tuple(sgr.export_image(m(B, 3, h, w), kind, size=(h, w)).shape) == (B, h, w, 3)
    assert tuple(sgr.export_image(m(B, 1, h, w), "image").shape) == (B, h, w, 3)      # one channel, written three times
    env = m(2, 3, 7, 9, 8, 16)
    mo = sgr.export_env_mosaic(env, nrows=3, ncols=4)
    assert tuple(mo.shape) == (2, 37, 86, 3) and mo.dtype == torch.uint8
    assert tuple(sgr.export_env_mosaic(m(1, 3, 120, 160, 8, 16), nrows=24, ncols=16).shape) == (1, 217, 273, 3)
    hw = sgr.export_env_hwc(env)
    assert tuple(hw.shape) == (2, 7, 9, 8, 16, 3) and hw.dtype == torch.float32
    preds = dict(albedo=[m(1, 3, h, w)] * 2, normal=[m(1, 3, h, w)], rough=[m(1, 1, h, w)], depth=[m(1, 1, h, w)], albedoBS=[m(1, 3, h, w)], roughBS=[m(1, 1, h, w)],
                 depthBS=[m(1, 1, h, w)], rendered=[m(1, 3, h, w)], shading=[m(1, 3, 4, 5)], envmaps=[m(1, 3, 24, 32, 8, 16)])
    out = sgr.export_predictions(preds, (9, 13), cAlbedos=[0.8])
    assert sorted(out) == sorted(["albedo0.png", "albedo1.png", "normal0.png", "rough0.png", "depth0.png", "albedoBS0.png", "roughBS0.png", "depthBS0.png", "rendered0.png",
                                  "shading0.png", "envmap0.npz", "envmap0.png"])
    assert tuple(out["albedo1.png"].shape) == (1, 9, 13, 3) and tuple(out["shading0.png"].shape) == (1, 4, 5, 3) and tuple(out["depthBS0.png"].shape) == (1, 9, 13, 1)
    assert tuple(out["envmap0.npz"].shape) == (1, 24, 32, 8, 16, 3) and tuple(out["envmap0.png"].shape) == (1, 24 * 9 + 1, 16 * 17 + 1, 3)
    for name in ("export_image", "export_env_mosaic", "export_env_hwc"):
        for key in ("Meta", "CUDA", "CPU", "AutocastCUDA"):      # AutocastCUDA: the fp32 rule
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", key), (name, key)
    assert sgr.EXPORT_KINDS == {k: i for i, k in enumerate(K.KINDS)}


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_wrapper_and_operator_refusals():
    ops = torch.ops.sgrender
    x3, x1, env = m(2, 3, 4, 6), m(2, 1, 4, 6), m(2, 3, 7, 9, 8, 16)
    for call in (lambda: sgr.export_image(torch.zeros(1, 3, 2, 2), "albedo"), lambda: sgr.export_env_mosaic(torch.zeros(1, 3, 2, 2, 2, 2), 1, 1),
                 lambda: sgr.export_env_hwc(torch.zeros(1, 3, 2, 2, 2, 2)), lambda: ops.export_image(torch.zeros(1, 3, 2, 2), 0, None, None, False)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match="x must be fp32"):
        sgr.export_image(m(2, 3, 4, 6, dtype=torch.float16), "albedo")
    with pytest.raises(RuntimeError, match="x must be fp32"):
        ops.export_image(m(2, 3, 4, 6, dtype=torch.float64), 1, None, None, False)
    with pytest.raises(RuntimeError, match=r"non-empty \[B,C,h,w\]"):
        sgr.export_image(m(3, 4, 6), "normal")
    with pytest.raises(RuntimeError, match=r"non-empty \[B,C,h,w\]"):
        sgr.export_image(m(0, 3, 4, 6), "normal")
    for kind, x, want in (("albedo", x1, "3"), ("normal", x1, "3"), ("rendered", x1, "3"), ("shading", x1, "3"), ("rough", x3, "1"), ("depth", x3, "1"), ("image", m(2, 2, 4, 6), "1 or 3"),
                          ("image_gamma", m(2, 4, 4, 6), "1 or 3")):
        with pytest.raises(RuntimeError, match=rf"export_image\({kind}\): this kind takes C = {want}"):
            sgr.export_image(x, kind)
    for size in ((0, 5), (5, 0), (-1, 5), (5,), (1, 2, 3)):
        with pytest.raises(RuntimeError, match="size must be two positive integers"):
            sgr.export_image(x3, "albedo", size=size)
    for size in ([0, 5], [5, 0], [5]):
        with pytest.raises(RuntimeError, match="size must be two positive integers"):
            ops.export_image(x3, 0, size, None, False)
    with pytest.raises(RuntimeError, match="written at the source's size"):
        sgr.export_image(x3, "shading", size=(8, 12))
    with pytest.raises(RuntimeError, match="written at the source's size"):
        ops.export_image(x1, 6, [8, 12], None, False)
    with pytest.raises(RuntimeError, match="unknown kind"):
        sgr.export_image(x3, "diffuse")
    with pytest.raises(RuntimeError, match="unknown kind"):
        ops.export_image(x3, 8, None, None, False)
    with pytest.raises(RuntimeError, match="one value per image"):
        sgr.export_image(x3, "albedo", scale=[0.5, 0.6, 0.7])
    with pytest.raises(RuntimeError, match="one value per image"):
        ops.export_image(x3, 0, None, m(3), False)
    with pytest.raises(RuntimeError, match="scale must be fp32"):
        ops.export_image(x3, 0, None, m(2, dtype=torch.float64), False)
    with pytest.raises(RuntimeError, match="belongs to the albedo kind"):
        sgr.export_image(x3, "normal", scale=[0.5, 0.6])
    with pytest.raises(RuntimeError, match="belongs to the albedo kind"):
        ops.export_image(x3, 1, None, m(2), False)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        sgr.export_image(np.zeros((1, 3, 2, 2), np.float32), "albedo")
    # env images
    with pytest.raises(RuntimeError, match="divides by zero"):
        sgr.export_env_mosaic(env, nrows=8, ncols=4)
    with pytest.raises(RuntimeError, match="divides by zero"):
        sgr.export_env_mosaic(env, nrows=3, ncols=10)
    with pytest.raises(RuntimeError, match="must be positive"):
        sgr.export_env_mosaic(env, nrows=0, ncols=4)
    with pytest.raises(RuntimeError, match="gap not negative"):
        sgr.export_env_mosaic(env, nrows=3, ncols=4, gap=-1)
    for bad in (m(2, 4, 7, 9, 8, 16), m(2, 1, 7, 9, 8, 16), m(2, 3, 7, 9, 8), m(0, 3, 7, 9, 8, 16)):
        with pytest.raises(RuntimeError, match=r"env must be a non-empty \[B,3,R,C,eh,ew\]"):
            sgr.export_env_mosaic(bad, 1, 1)
        with pytest.raises(RuntimeError, match=r"env must be a non-empty \[B,3,R,C,eh,ew\]"):
            sgr.export_env_hwc(bad)
    with pytest.raises(RuntimeError, match="env must be fp32"):
        sgr.export_env_hwc(m(2, 3, 7, 9, 8, 16, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="env must be fp32"):
        sgr.export_env_mosaic(m(2, 3, 7, 9, 8, 16, dtype=torch.float64), 1, 1)


def test_c_abi_refusals():
    """refused before anything is launched: the pointers are fake"""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    st4, st6 = (ctypes.c_longlong * 4)(72, 24, 6, 1), (ctypes.c_longlong * 6)(1, 1, 1, 1, 1, 1)
    err = lambda: lib.sgr_last_error().decode()
    base = dict(x=p, st=st4, scale=None, out=p, ws=p, kind=0, B=1, C=3, h=4, w=6, nh=8, nw=12, bgr=0, stream=None)
    img = lambda **k: lib.sgr_export_image(*{**base, **k}.values())
    assert img(x=None) == -1 and "sgr_export_image: NULL tensor" in err()
    assert img(out=None) == -1 and "NULL tensor" in err()
    assert img(st=None) == -1 and "NULL tensor" in err()
    assert img(kind=8) == -1 and "unknown kind" in err()
    assert img(kind=-1) == -1 and "unknown kind" in err()
    assert img(nh=0) == -1 and "non-positive size" in err()
    assert img(w=-3) == -1 and "non-positive size" in err()
    for kind, C in ((0, 1), (1, 1), (2, 3), (3, 3), (4, 1), (5, 1), (6, 2), (7, 4)):
        assert img(kind=kind, C=C, nh=4, nw=6) == -1 and "wrong channel count" in err(), (kind, C)
    for kind in (5, 6, 7):
        assert img(kind=kind) == -1 and "no resize" in err()
    assert img(kind=1, scale=p) == -1 and "belongs to the albedo kind" in err()
    assert img(kind=3, C=1, ws=None) == -1 and "NULL workspace" in err()
    assert img(B=65536) == -2 and "out of range" in err() and "cv2.resize" in err()
    assert img(h=32768, w=32768) == -2 and "out of range" in err()
    assert lib.sgr_export_image_workspace_floats(0, 4) == 0 and lib.sgr_export_image_workspace_floats(3, 4) == 256
    assert lib.sgr_export_image_workspace_floats(4, 1) == 64 and lib.sgr_export_image_workspace_floats(5, 2) == 128 and lib.sgr_export_image_workspace_floats(6, 2) == 0
    assert lib.sgr_export_image_workspace_floats(8, 1) < 0 and lib.sgr_export_image_workspace_floats(0, 0) < 0
    mos = lambda env=p, st=st6, out=p, B=1, R=7, C=9, eh=8, ew=16, nrows=3, ncols=4, gap=1: lib.sgr_export_env_mosaic(env, st, out, B, R, C, eh, ew, nrows, ncols, gap, 0, None)
    assert mos(env=None) == -1 and "sgr_export_env_mosaic: NULL tensor" in err()
    assert mos(R=0) == -1 and "non-positive size" in err()
    assert mos(nrows=0) == -1 and "must be positive" in err()
    assert mos(gap=-1) == -1 and "gap not negative" in err()
    assert mos(nrows=8) == -1 and "divides by zero" in err()
    assert mos(ncols=10) == -1 and "divides by zero" in err()
    assert mos(B=65536) == -2 and "writeEnvToFile" in err()
    hwc = lambda env=p, out=p, B=1, R=2, C=2, eh=8, ew=16: lib.sgr_export_env_hwc(env, out, B, R, C, eh, ew, 1, None)
    assert hwc(out=None) == -1 and "sgr_export_env_hwc: NULL tensor" in err()
    assert hwc(eh=0) == -1 and "non-positive size" in err()
    assert hwc(R=65536, C=65536) == -2 and "np.ascontiguousarray" in err()


# ---- the kernels' decisions on the host, under sanitizers ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("export") / "export_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           os.path.join(ROOT, "tests", "host_emul", "export_main.cpp"), "-o", exe])
    return exe


def run_host(exe, tmp_path, payload):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(payload)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return open(dst, "rb").read()


def host_image(exe, tmp_path, x, kind, size, scale, bgr):
    B, C, h, w = x.shape
    nh, nw = size if size is not None else (h, w)
    payload = struct.pack("10i", 0, sgr.EXPORT_KINDS[kind], B, C, h, w, nh, nw, int(bgr), int(scale is not None)) + np.ascontiguousarray(x, np.float32).tobytes()
    if scale is not None:
        payload += np.ascontiguousarray(scale, np.float32).tobytes()
    out = np.frombuffer(run_host(exe, tmp_path, payload), np.uint8)
    return out.reshape(B, nh, nw, 3 if kind.startswith("image") else C)


def test_host_build_of_the_kernel_logic_gives_the_fixtures_bytes(host_program, tmp_path):
    for name in IMAGE_CASES:
        for z, kind, key, x, size, scale in fixture_sets(name):
            got = host_image(host_program, tmp_path, x, kind, size, scale, False)
            K.check_bytes(got, t64_of(x, kind, size, scale), float(z["e_t_" + key]), f"host {name} {key}")
            assert np.array_equal(host_image(host_program, tmp_path, x, kind, size, scale, True), got[..., ::-1]), (name, key)
    z = fixture("env")
    for tag in ("a", "b"):
        env, (nrows, ncols, gap) = z["env_" + tag], (int(v) for v in z["cfg_" + tag])
        B, _, R, C, eh, ew = env.shape
        raw = run_host(host_program, tmp_path, struct.pack("10i", 1, B, R, C, eh, ew, nrows, ncols, gap, 0) + env.tobytes())
        Hm, Wm = struct.unpack("2i", raw[:8])
        assert (Hm, Wm) == K.mosaic_geometry(R, C, eh, ew, nrows, ncols, gap)[4:]
        K.check_bytes(np.frombuffer(raw[8:], np.uint8).reshape(B, Hm, Wm, 3), K.env_mosaic_t(env, nrows, ncols, gap, clip=False), float(z["e_t_mosaic_" + tag]), f"host mosaic {tag}")


def test_host_build_of_the_index_rule_and_the_edge_values(host_program, tmp_path):
    for n_in, n_out in ((1, 1), (1, 5), (5, 1), (7, 11), (13, 10), (41, 60), (160, 320), (12, 12), (90, 5)):
        raw = run_host(host_program, tmp_path, struct.pack("3i", 2, n_in, n_out))
        s, f = np.frombuffer(raw[:4 * n_out], np.int32), np.frombuffer(raw[4 * n_out:], np.float32)
        ws, wf = K.src_of(n_in, n_out)
        assert np.array_equal(s, ws) and np.array_equal(f, wf), (n_in, n_out)
    # NaN -> 0, saturation both ways, the 1e-10 floor of an all-zero depth image
    x = np.array([np.nan, -3.0, 0.0, 1.0, 7.0, np.inf], np.float32).reshape(1, 1, 2, 3)
    assert host_image(host_program, tmp_path, x, "rough", None, None, False).reshape(-1).tolist() == [0, 0, 127, 255, 255, 255]
    assert host_image(host_program, tmp_path, np.zeros((1, 1, 2, 2), np.float32), "depth", None, None, False).reshape(-1).tolist() == [255] * 4
    assert host_image(host_program, tmp_path, x.clip(0, 1).repeat(3, 1)[:, :, :, 1:], "image", None, None, False).shape == (1, 2, 2, 3)
