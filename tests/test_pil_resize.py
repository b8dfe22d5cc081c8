"""CPU: PIL's antialiased resize (sgr.pil_resize, sgr.iiw_resize_crop, sgr.loader_resize) without a GPU -- the numpy checker against the bytes
the installed Pillow wrote into the fixtures and, where PIL imports, against live ``Image.resize``; the C table builder against the stored
tables; the kernels' per-thread bodies (csrc/sgr_pil_resize.h) compiled for the host as a stand-alone program under
-fsanitize=address,undefined against the fixtures' bytes on both routes; the IIW geometry; Meta shapes, every refusal through the wrapper, the
operator and the C entry; the route ``auto`` takes.  Every comparison of bytes and of table entries is ``==``."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import pil_resize_checker as K
from conftest import GOLDEN_DIR, ROOT
from inverserenderingofindoorscene_amd import _lib

TILED, TWO_PASS, ROUTE, WINDOWS, IIW_CS = K.TILED, K.TWO_PASS, K.ROUTE, K.WINDOWS, K.IIW_CS


def fixture(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g31_pil_resize_{name}.npz"))


def case_of(name):
    return int(name[1:].split("_")[0])


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    return pkg


# ---- the checker ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.fixture_names())
def test_checker_equals_every_fixture(name):
    z = fixture(name)
    H, W, out_w, out_h = (int(v) for v in z["geom"])
    assert (H, W, out_w, out_h) == K.CASES[case_of(name)][:4]
    seen = 0
    for tag, im, filt, want in K.entries(z):
        assert np.array_equal(K.resize(im, (out_w, out_h), filt), want), (name, tag)
        seen += 1
    assert seen > 0
    for filt in K.CASES[case_of(name)][4]:
        for axis, (n_in, n_out) in (("h", (W, out_w)), ("v", (H, out_h))):
            b, k, _ = K.table(n_in, n_out, filt)
            assert np.array_equal(b, z[f"{axis}b_{filt}"]) and np.array_equal(k, z[f"{axis}k_{filt}"])


def test_fixtures_cover_the_cases_and_both_clamps():
    names = K.fixture_names()
    assert sorted(set(case_of(n) for n in names)) == list(range(1, 14))
    z = fixture("c12_C3_binary")
    out = z["out_3_binary_lanczos"]
    assert out.min() == 0 and out.max() == 255 and tuple(out.shape) == (240, 320, 3)
    # the integer ranges DESIGN.md section 8p quotes: |k| below 2^23 (the 24-bit multiply), 255 sum |k| + 2^21 below 2^31
    worst_k = worst_sum = 0
    for name in names:
        z = fixture(name)
        for key in z.files:
            if key[:3] in ("hk_", "vk_"):
                a, s = K.table_stats(z[key])
                worst_k, worst_sum = max(worst_k, a), max(worst_sum, s)
    assert worst_k < 2 ** 23 and (1 << 21) + 255 * worst_sum < 2 ** 31


def test_checker_equals_live_pil():
    Image = pytest.importorskip("PIL.Image")
    codes = {"lanczos": Image.Resampling.LANCZOS, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC, "box": Image.Resampling.BOX,
             "hamming": Image.Resampling.HAMMING}
    assert {k: int(v) for k, v in codes.items()} == K.FILTERS
    rng = np.random.default_rng(31)
    for H, W, out_w, out_h in [(48, 64, 32, 24), (37, 53, 20, 17), (30, 40, 57, 41), (33, 47, 47, 20), (33, 47, 30, 33), (5, 7, 3, 2), (2, 3, 1, 1), (19, 23, 23, 19),
                               (61, 45, 7, 11), (9, 100, 33, 27)]:
        for C in (1, 3):
            im = rng.integers(0, 256, (H, W, C), dtype=np.uint8) if (H + C) % 2 else (rng.integers(0, 2, (H, W, C), dtype=np.uint8) * 255).astype(np.uint8)
            pim = Image.fromarray(im[:, :, 0], "L") if C == 1 else Image.fromarray(im, "RGB")
            for filt, code in codes.items():
                want = np.asarray(pim.resize((out_w, out_h), code)).reshape(out_h, out_w, C)
                assert np.array_equal(K.resize(im, (out_w, out_h), filt), want), (H, W, out_w, out_h, C, filt)


def test_checker_windows_are_slices():
    z = fixture("c2")
    im = z["im_3_noise"]
    for filt in ("lanczos", "box"):
        full = z[f"out_3_noise_{filt}"]
        for r0, c0, h, w in WINDOWS[2]:
            assert np.array_equal(K.resize(im, (20, 17), filt, (r0, c0, h, w)), full[r0:r0 + h, c0:c0 + w])


# ---- the C table builder --------------------------------------------------------------------------------------------------------------------

def c_table(lib, n_in, n_out, code):
    n = lib.sgr_pil_resize_table_ints(n_in, n_out, code)
    assert n > 0
    buf = (ctypes.c_int * n)()
    assert lib.sgr_pil_resize_table(n_in, n_out, code, buf) == 0, lib.sgr_last_error()
    return np.frombuffer(buf, np.int32).copy()


@pytest.mark.parametrize("name", K.fixture_names())
def test_c_table_builder_equals_the_stored_tables(name):
    lib = _lib.load()
    z = fixture(name)
    H, W, out_w, out_h = (int(v) for v in z["geom"])
    for filt in K.CASES[case_of(name)][4]:
        for axis, (n_in, n_out) in (("h", (W, out_w)), ("v", (H, out_h))):
            t = c_table(lib, n_in, n_out, K.FILTERS[filt])
            b, k = z[f"{axis}b_{filt}"], z[f"{axis}k_{filt}"]
            ksize = k.shape[1]
            assert t[:4].tolist() == [ksize, 0, n_in, n_out] and ksize == K.ksize_of(n_in, n_out, filt)
            assert len(t) == 4 + 2 * n_out + n_out * ksize
            assert np.array_equal(t[4:4 + 2 * n_out].reshape(n_out, 2), b) and np.array_equal(t[4 + 2 * n_out:].reshape(n_out, ksize), k)


# ---- the stand-alone host program -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pil_resize") / "pil_resize_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           os.path.join(ROOT, "tests", "host_emul", "pil_resize_main.cpp"), "-o", exe])
    return exe


def run_host(exe, tmp_path, im, size, filt, path, window=None, misalign=0, tables=False):
    """-> the bytes [bn,h,w,C] (and the tables' ints), or None where `tiled` does not fit"""
    bn, H, W, C = im.shape
    out_w, out_h = size
    r0, c0, h, w = window if window is not None else (0, 0, out_h, out_w)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("14i", bn, H, W, C, out_h, out_w, r0, c0, h, w, K.FILTERS[filt], path, misalign, int(tables)) + np.ascontiguousarray(im).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    if r.returncode == 3:
        return None
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    buf = open(dst, "rb").read()
    n = bn * h * w * C
    out = np.frombuffer(buf, np.uint8, n).reshape(bn, h, w, C)
    return (out, np.frombuffer(buf, np.int32, (len(buf) - n) // 4, n)) if tables else out


@pytest.mark.parametrize("name", K.fixture_names())
def test_host_program_reproduces_the_fixtures_on_both_routes(host_program, tmp_path, name):
    """the same per-thread bodies as the kernels, over exactly-sized heap buffers: clean under the sanitizers means that no index left the
    source, the workspace, the LDS tiles or the output, and that every 32-bit access was aligned"""
    z = fixture(name)
    H, W, out_w, out_h = (int(v) for v in z["geom"])
    n = case_of(name)
    for tag, im, filt, want in K.entries(z):
        for path in (TWO_PASS, TILED):
            for misalign in (0, 1) if n in K.SMALL else (3,):
                got = run_host(host_program, tmp_path, im[None], (out_w, out_h), filt, path, misalign=misalign)
                if path == TILED and ROUTE[n] != TILED:
                    assert got is None, (name, tag)
                    continue
                assert got is not None and np.array_equal(got[0], want), (name, tag, path, misalign)


def test_host_program_windows_batches_and_tables(host_program, tmp_path):
    for n, name, key in ((2, "c2", "3_noise"), (8, "c8_C3_noise", "3_noise"), (8, "c8_C1_binary", "1_binary")):
        z = fixture(name)
        H, W, out_w, out_h = (int(v) for v in z["geom"])
        im, full = z["im_" + key], z[f"out_{key}_lanczos"]
        for win in WINDOWS[n]:
            r0, c0, h, w = win
            for path in (TWO_PASS, TILED):
                got = run_host(host_program, tmp_path, im[None], (out_w, out_h), "lanczos", path, window=win, misalign=2)
                assert np.array_equal(got[0], full[r0:r0 + h, c0:c0 + w]), (name, win, path)
    z = fixture("c13_C3_noise")
    for cs in IIW_CS:
        for path in (TWO_PASS, TILED):
            got = run_host(host_program, tmp_path, z["im_3_noise"][None], (361, 240), "lanczos", path, window=(0, cs, 240, 320))
            assert np.array_equal(got[0], z["out_3_noise_lanczos"][:, cs:cs + 320]), (cs, path)
    # a batch: image b is what it is alone; the tables the program built are the stored ones
    z = fixture("c2")
    batch = np.stack([z["im_3_noise"], z["im_3_smooth"], z["im_3_binary"]])
    for path in (TWO_PASS, TILED):
        got, tabs = run_host(host_program, tmp_path, batch, (20, 17), "bicubic", path, tables=True)
        for b, kind in enumerate(K.KINDS):
            assert np.array_equal(got[b], z[f"out_3_{kind}_bicubic"]), (path, kind)
        nh = 4 + 2 * 20 + 20 * z["hk_bicubic"].shape[1]
        assert np.array_equal(tabs[4 + 40:nh].reshape(20, -1), z["hk_bicubic"]) and np.array_equal(tabs[nh + 4 + 34:].reshape(17, -1), z["vk_bicubic"])
    # a horizontal ksize between 17 and 32 (taps from the LDS table, not from registers) and one above 32 (no tiles)
    rng = np.random.default_rng(5)
    im = rng.integers(0, 256, (60, 300, 3), dtype=np.uint8)
    want = K.resize(im, (100, 40), "lanczos")
    assert K.ksize_of(300, 100, "lanczos") == 19
    for path in (TWO_PASS, TILED):
        assert np.array_equal(run_host(host_program, tmp_path, im[None], (100, 40), "lanczos", path, misalign=1)[0], want), path
    assert run_host(host_program, tmp_path, im[None], (25, 40), "lanczos", TILED) is None and K.ksize_of(300, 25, "lanczos") == 73


# ---- the route ------------------------------------------------------------------------------------------------------------------------------

def test_tiled_fit_and_auto_route_per_fixture_geometry():
    lib = _lib.load()
    tiles = lambda h, w: -(-h // 16) * -(-w // 64)
    for n, (H, W, out_w, out_h, filters) in K.CASES.items():
        for C in (1, 3):
            for filt in filters:
                code = K.FILTERS[filt]
                assert lib.sgr_pil_resize_tiled_fits(H, W, C, out_h, out_w, None, code) == int(ROUTE[n] == TILED), (n, C, filt)
                # auto: tiled where it fits and the launch has at least 256 tiles (where it measured faster beyond the spread)
                for bn in (1, 3, 4, 16, 300):
                    want = TILED if ROUTE[n] == TILED and bn * tiles(out_h, out_w) >= 256 else TWO_PASS
                    assert lib.sgr_pil_resize_route(bn, H, W, C, out_h, out_w, None, code) == want, (n, C, filt, bn)
    assert lib.sgr_pil_resize_route(1, 480, 640, 3, 240, 320, None, 1) == TWO_PASS and lib.sgr_pil_resize_route(3, 480, 640, 3, 240, 320, None, 1) == TWO_PASS
    assert lib.sgr_pil_resize_route(4, 480, 640, 3, 240, 320, None, 1) == TILED and lib.sgr_pil_resize_route(16, 480, 640, 3, 240, 320, None, 1) == TILED
    assert K.ksize_of(131, 9, "lanczos") == 89      # case 11: the taps alone rule the tiles out
    win = (ctypes.c_int * 4)(0, 20, 240, 320)
    assert lib.sgr_pil_resize_tiled_fits(341, 512, 3, 240, 361, win, 1) == 1 and lib.sgr_pil_resize_route(1, 341, 512, 3, 240, 361, win, 1) == TWO_PASS
    # 3x down, RGB: a 16 x 64 tile reads 66 rows of 636 bytes -- beyond the 24 KiB source tile
    assert lib.sgr_pil_resize_tiled_fits(720, 960, 3, 240, 320, None, 1) == 0 and lib.sgr_pil_resize_route(64, 720, 960, 3, 240, 320, None, 1) == TWO_PASS
    # the workspace of the two_pass route: the rows the window reads times the window's row rounded up to 4 bytes; none for a single pass
    ya, yb = K.needed_rows(341, 240, "lanczos", 0, 240)
    assert lib.sgr_pil_resize_workspace_bytes(2, 341, 512, 3, 240, 361, win, 1) == 2 * (yb - ya) * 960
    ya, yb = K.needed_rows(37, 17, "lanczos", 3, 9)
    win2 = (ctypes.c_int * 4)(3, 4, 9, 11)
    assert lib.sgr_pil_resize_workspace_bytes(1, 37, 53, 3, 17, 20, win2, 1) == (yb - ya) * 36 and yb - ya < 37
    assert lib.sgr_pil_resize_workspace_bytes(1, 33, 47, 3, 20, 47, None, 1) == 0 and lib.sgr_pil_resize_workspace_bytes(1, 33, 47, 3, 33, 47, None, 1) == 0


# ---- the IIW geometry -----------------------------------------------------------------------------------------------------------------------

def test_iiw_geometry_equals_the_references_expressions_over_a_sweep():
    from inverserenderingofindoorscene_amd.pil_resize import iiw_geometry
    seen = set()
    for imH, imW in ((240, 320), (480, 640), (100, 100), (7, 3)):
        for nh in list(range(1, 40)) + [240, 341, 375, 500, 512, 683, 1024]:
            for nw in list(range(1, 40)) + [320, 341, 375, 500, 512, 683, 1024]:
                # iiwDataLoader.py:115-133, verbatim
                scaleW = float(imW) / float(nw)
                scaleH = float(imH) / float(nh)
                if scaleW > scaleH:
                    newW = imW
                    newH = int(np.ceil(scaleW * nh))
                    gap, along = newH - imH, "rows"
                else:
                    newH = imH
                    newW = int(np.ceil(scaleH * nw))
                    gap, along = newW - imW, "columns"
                assert newW >= imW and newH >= imH
                assert iiw_geometry(nh, nw, imH, imW) == (newH, newW, gap, along) == K.iiw_geometry(nh, nw, imH, imW)
                seen.add(along)
    assert seen == {"rows", "columns"} and iiw_geometry(341, 512, 240, 320) == (240, 361, 41, "columns")


# ---- Meta kernels and refusals --------------------------------------------------------------------------------------------------------------

def meta(*shape, dtype=torch.uint8):
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_meta_shapes_and_dtypes(sgr):
    out = sgr.pil_resize(meta(4, 480, 640, 3), (320, 240))
    assert tuple(out.shape) == (4, 240, 320, 3) and out.dtype == torch.uint8 and out.device.type == "meta"
    assert tuple(sgr.pil_resize(meta(37, 53, 1), (20, 17), "box").shape) == (17, 20, 1)
    assert tuple(sgr.pil_resize(meta(2, 37, 53, 3), (20, 17), window=(3, 4, 9, 11), path="two_pass").shape) == (2, 9, 11, 3)
    assert tuple(sgr.pil_resize(meta(33, 47, 3), (47, 33), 3).shape) == (33, 47, 3)      # PIL's integer code; equal sizes: a copy
    assert tuple(torch.ops.sgrender.pil_resize(meta(5, 7, 3), 3, 2).shape) == (2, 3, 3)
    crop, newH, newW, rs, cs = sgr.iiw_resize_crop(meta(341, 512, 3), 240, 320, 20)
    assert tuple(crop.shape) == (240, 320, 3) and (newH, newW, rs, cs) == (240, 361, 0, 20)
    crop, newH, newW, rs, cs = sgr.iiw_resize_crop(meta(512, 341, 3), 240, 320, 7)
    assert tuple(crop.shape) == (240, 320, 3) and (newH, newW, rs, cs) == (481, 320, 7, 0)
    raw = dict(seg=meta(2, 480, 640, 3), albedo=meta(2, 480, 640, 3), normal=meta(2, 480, 640, 3), rough=meta(2, 480, 640, 1), im=meta(2, 240, 320, 3, dtype=torch.float32), name=["a", "b"])
    got = sgr.loader_resize(raw, (320, 240))
    assert sorted(got) == sorted(raw) and got["im"] is raw["im"] and got["name"] is raw["name"]
    assert [tuple(got[k].shape) for k in ("seg", "albedo", "normal", "rough")] == [(2, 240, 320, 3)] * 3 + [(2, 240, 320, 1)]
    for name in ("pil_resize", "iiw_resize_crop", "loader_resize"):
        assert name in sgr.__all__
    for key in ("Meta", "CUDA", "CPU", "AutocastCUDA"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("sgrender::pil_resize", key), key
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("sgrender::pil_resize", "Autograd")


REFUSALS = [      # (arguments of the wrapper on a Meta tensor, a piece of the message)
    (dict(im=meta(8, 8, 3, dtype=torch.float32)), "must be uint8"),
    (dict(im=meta(8, 8, 3, dtype=torch.int32)), "must be uint8"),
    (dict(im=meta(8, 8, 4)), "premultiplied-alpha"),
    (dict(im=meta(2, 8, 8, 2)), "premultiplied-alpha"),
    (dict(im=meta(8, 8)), r"\[H,W,C\] or \[bn,H,W,C\]"),
    (dict(im=meta(0, 8, 3)), "zero-sized input"),
    (dict(im=meta(0, 8, 8, 3)), "zero-sized input"),
    (dict(size=(0, 4)), "zero-sized or negative output"),
    (dict(size=(4, -1)), "zero-sized or negative output"),
    (dict(window=(0, 0, 5, 4)), "leaves the resized image"),
    (dict(window=(-1, 0, 2, 2)), "leaves the resized image"),
    (dict(window=(0, 3, 2, 2)), "leaves the resized image"),
    (dict(window=(0, 0, 0, 2)), "zero-sized"),
    (dict(window=(0, 0, 2)), "window must be"),
    (dict(filter="nearest"), "different PIL code path"),
    (dict(filter=0), "different PIL code path"),
    (dict(filter="gauss"), "unknown filter"),
    (dict(filter=6), "unknown filter"),
    (dict(path="fast"), "unknown path"),
    (dict(reducing_gap=2.0), "reducing_gap is not offered"),
    (dict(box=(0, 0, 4, 4)), "source box is not offered"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_refusals_through_the_wrapper_and_the_operator(sgr, change, message):
    args = dict(im=meta(8, 8, 3), size=(4, 4), filter="lanczos", window=None, path="auto")
    args.update(change)
    im = args.pop("im")
    size = args.pop("size")
    with pytest.raises(RuntimeError, match=message):
        sgr.pil_resize(im, size, **args)
    if "box" in change or "reducing_gap" in change or isinstance(args["filter"], int):
        return      # the operator has no such argument, and takes the filter by name
    with pytest.raises(RuntimeError, match=message):
        torch.ops.sgrender.pil_resize(im, size[0], size[1], args["filter"], args["window"], args["path"])


def test_cpu_tensors_and_the_wrappers_own_refusals(sgr):
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.pil_resize(torch.zeros(8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(RuntimeError, match="must be a tensor"):
        sgr.pil_resize(np.zeros((8, 8, 3), np.uint8), (4, 4))
    with pytest.raises(RuntimeError, match=r"size must be \(width, height\)"):
        sgr.pil_resize(meta(8, 8, 3), 4)
    with pytest.raises(RuntimeError, match=r"offset 42 is outside 0 .. gap = 41"):
        sgr.iiw_resize_crop(meta(341, 512, 3), 240, 320, 42)
    with pytest.raises(RuntimeError, match="outside 0 .. gap"):
        sgr.iiw_resize_crop(meta(341, 512, 3), 240, 320, -1)
    with pytest.raises(RuntimeError, match=r"one photograph \[H,W,C\]"):
        sgr.iiw_resize_crop(meta(1, 341, 512, 3), 240, 320, 0)
    with pytest.raises(RuntimeError, match="premultiplied-alpha"):
        sgr.iiw_resize_crop(meta(341, 512, 4), 240, 320, 0)
    with pytest.raises(RuntimeError, match="albedo must be uint8"):
        sgr.loader_resize(dict(albedo=meta(1, 8, 8, 3, dtype=torch.float32)), (4, 4))


C_REFUSALS = [      # (changed arguments of sgr_pil_resize_u8, NULL pointers, code, a piece of the message)
    ({}, ["src"], -1, "NULL tensor"),
    (dict(H=0), [], -1, "zero-sized or negative"),
    (dict(outW=0), [], -1, "zero-sized or negative"),
    (dict(bn=-1), [], -1, "zero-sized or negative"),
    (dict(C=4), [], -2, "premultiplied-alpha"),
    (dict(C=2), [], -2, "premultiplied-alpha"),
    (dict(filter=0), [], -2, "nearest"),
    (dict(filter=9), [], -1, "unknown filter"),
    (dict(window=(0, 0, 5, 4)), [], -1, "leaves the resized image"),
    (dict(window=(0, -1, 4, 4)), [], -1, "leaves the resized image"),
    (dict(window=(0, 0, 0, 4)), [], -1, "zero-sized"),
    (dict(path=3), [], -1, "path must be"),
    ({}, ["htable"], -1, "NULL table"),
    ({}, ["vtable"], -1, "NULL table"),
    (dict(path=1), ["workspace"], -1, "NULL workspace"),
    (dict(H=97, W=131, outH=7, outW=9, path=2), [], -2, "does not fit the tiles"),
    (dict(outH=8, path=2), [], -2, "does not fit the tiles"),      # a single pass: no tiles
    (dict(bn=65536), [], -2, "out of range"),
]


@pytest.mark.parametrize("change,nulls,code,message", C_REFUSALS, ids=[m + str(i) for i, (_, _, _, m) in enumerate(C_REFUSALS)])
def test_refusals_through_the_c_entry(change, nulls, code, message):
    """every call is refused before anything is launched: the pointers are fake"""
    lib = _lib.load()
    a = dict(bn=1, H=8, W=8, C=3, outH=4, outW=4, window=None, filter=1, path=0)
    a.update(change)
    fake = lambda name: None if name in nulls else ctypes.c_void_p(4096)
    win = (ctypes.c_int * 4)(*a["window"]) if a["window"] is not None else None
    rc = lib.sgr_pil_resize_u8(fake("src"), a["bn"], a["H"], a["W"], a["C"], fake("dst"), a["outH"], a["outW"], win, a["filter"], fake("htable"), fake("vtable"),
                               fake("workspace"), a["path"], None)
    assert rc == code and message.encode() in lib.sgr_last_error(), (rc, lib.sgr_last_error())
    if not nulls and "path" not in change:      # the queries share the check
        assert lib.sgr_pil_resize_workspace_bytes(a["bn"], a["H"], a["W"], a["C"], a["outH"], a["outW"], win, a["filter"]) == code
        assert message.encode() in lib.sgr_last_error()


def test_table_entry_refusals():
    lib = _lib.load()
    buf = (ctypes.c_int * 64)()
    for args, message in (((0, 4, 1), b"sizes must be"), ((4, 0, 1), b"sizes must be"), ((4, 4, 0), b"nearest"), ((4, 4, 7), b"unknown filter"), (((1 << 24) + 1, 4, 1), b"sizes must be")):
        assert lib.sgr_pil_resize_table_ints(*args) == -1 and message in lib.sgr_last_error()
        assert lib.sgr_pil_resize_table(*args, buf) == -1 and message in lib.sgr_last_error()
    assert lib.sgr_pil_resize_table(4, 4, 1, None) == -1 and b"NULL table" in lib.sgr_last_error()
    assert lib.sgr_pil_resize_table_ints(640, 320, 1) == 4 + 2 * 320 + 320 * 13
