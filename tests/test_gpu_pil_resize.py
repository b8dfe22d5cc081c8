"""GPU: PIL's antialiased resize on the device (sgr.pil_resize, sgr.iiw_resize_crop, sgr.loader_resize) -- every fixture's bytes, written by the
installed Pillow, with ``==`` on the two_pass route, on the tiled route wherever the geometry fits, and on auto; windows against slices; batch,
rerun, strides and alignment; the raw C entry (the 32-bit multiply included); HIP-graph capture after a warm-up call; and the two loaders'
compositions against values the existing checkers compute from PIL's bytes.  The GPU tests read fixtures and the numpy checker only: Pillow
may be missing on the machine."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loader_prep_checker as LK
import pil_resize_checker as K
import real_loader_checker as RK
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

PATHS = {K.TWO_PASS: "two_pass", K.TILED: "tiled"}


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = np.load(os.path.join(GOLDEN_DIR, f"g31_pil_resize_{name}.npz"))
    return _cache[name]


def case_of(name):
    return int(name[1:].split("_")[0])


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same(t, want):
    return t.dtype == torch.uint8 and tuple(t.shape) == want.shape and t.is_contiguous() and np.array_equal(t.cpu().numpy(), want)


def routes_of(n):
    return ("two_pass", "tiled", "auto") if K.ROUTE[n] == K.TILED else ("two_pass", "auto")


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.fixture_names())
def test_every_fixture_on_every_route(sgr, name):
    z = fixture(name)
    _, _, out_w, out_h = (int(v) for v in z["geom"])
    n = case_of(name)
    for tag, im, filt, want in K.entries(z):
        d = dev(im)
        for path in routes_of(n):
            assert same(sgr.pil_resize(d, (out_w, out_h), filt, path=path), want), (name, tag, path)
        if K.ROUTE[n] != K.TILED:
            with pytest.raises(RuntimeError, match="does not fit the tiles"):
                sgr.pil_resize(d, (out_w, out_h), filt, path="tiled")


def test_auto_takes_the_tiled_route_from_256_tiles_on_with_the_same_bytes(sgr):
    from inverserenderingofindoorscene_amd import _lib
    z = fixture("c12_C3_binary")      # the loader's own geometry: 75 tiles an image
    im, want = z["im_3_binary"], z["out_3_binary_lanczos"]
    lib = _lib.load()
    assert lib.sgr_pil_resize_route(4, 480, 640, 3, 240, 320, None, 1) == K.TILED and lib.sgr_pil_resize_route(1, 480, 640, 3, 240, 320, None, 1) == K.TWO_PASS
    d = dev(np.stack([im, im[::-1], im[:, ::-1], im]))
    out = sgr.pil_resize(d, (320, 240))
    assert same(out[0], want) and same(out[3], want) and same(out[1], K.resize(im[::-1], (320, 240)))
    assert torch.equal(out, sgr.pil_resize(d, (320, 240), path="two_pass")) and torch.equal(out, sgr.pil_resize(d, (320, 240), path="tiled"))


def test_windows_equal_slices_of_the_full_result(sgr):
    for n, name, key in ((2, "c2", "3_noise"), (2, "c2", "1_binary"), (8, "c8_C3_noise", "3_noise"), (8, "c8_C1_smooth", "1_smooth")):
        z = fixture(name)
        _, _, out_w, out_h = (int(v) for v in z["geom"])
        d, full = dev(z["im_" + key]), z[f"out_{key}_lanczos"]
        for r0, c0, h, w in K.WINDOWS[n]:
            for path in routes_of(n):
                assert same(sgr.pil_resize(d, (out_w, out_h), window=(r0, c0, h, w), path=path), full[r0:r0 + h, c0:c0 + w]), (name, (r0, c0, h, w), path)
    z = fixture("c13_C3_noise")      # the IIW geometry: 341 x 512 to newH 240, newW 361, the crop along the columns
    d, full = dev(z["im_3_noise"]), z["out_3_noise_lanczos"]
    for cs in K.IIW_CS:
        for path in routes_of(13):
            assert same(sgr.pil_resize(d, (361, 240), window=(0, cs, 240, 320), path=path), full[:, cs:cs + 320]), (cs, path)
    # windows of the single-pass and the copy geometries
    for name, size in (("c4", (47, 20)), ("c5", (30, 33)), ("c10", (47, 33))):
        z = fixture(name)
        d, full = dev(z["im_3_noise"]), z["out_3_noise_bicubic"]
        for win in ((0, 0, size[1], size[0]), (3, 5, 11, 13), (size[1] - 1, size[0] - 1, 1, 1)):
            r0, c0, h, w = win
            assert same(sgr.pil_resize(d, size, "bicubic", window=win), full[r0:r0 + h, c0:c0 + w]), (name, win)


def test_geometries_no_fixture_holds_against_the_checker(sgr):
    """a horizontal ksize of 19 (taps from the LDS table instead of registers), several tiles with ragged edges in both directions, an
    upscale along one axis with a reduction along the other, and a row of W C bytes that is no multiple of 4"""
    rng = np.random.default_rng(310)
    for (H, W, C), size, filt in (((60, 300, 3), (100, 40), "lanczos"), ((60, 300, 1), (100, 40), "lanczos"), ((150, 333, 3), (171, 77), "lanczos"),
                                  ((45, 50, 3), (131, 20), "bicubic"), ((70, 131, 1), (67, 90), "hamming"), ((40, 200, 3), (80, 39), "bilinear")):
        im = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        want = K.resize(im, size, filt)
        route = "tiled" if K.ksize_of(W, size[0], filt) <= 32 and K.ksize_of(H, size[1], filt) <= 32 else "two_pass"
        for path in ("two_pass", route, "auto"):
            assert same(sgr.pil_resize(dev(im), size, filt, path=path), want), (H, W, C, size, filt, path)
    assert K.ksize_of(300, 100, "lanczos") == 19


# ---- exact properties -----------------------------------------------------------------------------------------------------------------------

def test_batch_rerun_strides_and_alignment(sgr):
    z = fixture("c2")
    batch = np.stack([z["im_3_noise"], z["im_3_smooth"], z["im_3_binary"]])
    want = np.stack([z[f"out_3_{kind}_lanczos"] for kind in K.KINDS])
    d = dev(batch)
    for path in ("two_pass", "tiled"):
        out = sgr.pil_resize(d, (20, 17), path=path)
        assert same(out, want) and torch.equal(out, sgr.pil_resize(d, (20, 17), path=path))
        for b in range(3):      # an image does not depend on its batch
            assert torch.equal(sgr.pil_resize(d[b], (20, 17), path=path), out[b]) and torch.equal(sgr.pil_resize(d[b:b + 1], (20, 17), path=path)[0], out[b])
        # a non-contiguous input: column and channel slices of a wider, deeper batch
        wide = dev(np.concatenate([batch, batch[:, :, ::-1]], axis=2))[:, :, :53]
        assert not wide.is_contiguous() and same(sgr.pil_resize(wide, (20, 17), path=path), want)
        chw = dev(np.ascontiguousarray(batch.transpose(0, 3, 1, 2))).permute(0, 2, 3, 1)
        assert not chw.is_contiguous() and same(sgr.pil_resize(chw, (20, 17), path=path), want)
        # one, two and three bytes off a 4-byte boundary: the staging's byte path and the unaligned stores
        for off in (1, 2, 3):
            flat = torch.empty(batch.size + off, dtype=torch.uint8, device="cuda")
            flat[off:] = d.reshape(-1)
            v = flat[off:].view(batch.shape)
            assert v.data_ptr() % 4 == off and same(sgr.pil_resize(v, (20, 17), path=path), want)
    one = dev(z["im_1_noise"])
    assert same(sgr.pil_resize(one, (20, 17), "box"), z["out_1_noise_box"]) and same(sgr.pil_resize(one, (20, 17), 4), z["out_1_noise_box"])


def test_autocast_and_no_autograd(sgr):
    z = fixture("c1")
    d = dev(z["im_3_noise"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = sgr.pil_resize(d, (32, 24))
    assert same(out, z["out_3_noise_lanczos"]) and not out.requires_grad
    torch.library.opcheck(torch.ops.sgrender.pil_resize.default, (d, 32, 24), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.sgrender.pil_resize.default, (d, 32, 24, "bicubic", [2, 3, 7, 9], "two_pass"), test_utils=("test_schema", "test_faketensor"))


# ---- the raw C entry ------------------------------------------------------------------------------------------------------------------------

def host_table(lib, n_in, n_out, code):
    n = lib.sgr_pil_resize_table_ints(n_in, n_out, code)
    buf = (ctypes.c_int * n)()
    assert lib.sgr_pil_resize_table(n_in, n_out, code, buf) == 0, lib.sgr_last_error()
    return np.frombuffer(buf, np.int32).copy()


def test_raw_c_entry_with_its_own_tables_and_the_32_bit_multiply(sgr):
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    z = fixture("c2")
    H, W, out_w, out_h = (int(v) for v in z["geom"])
    batch = np.stack([z["im_3_noise"], z["im_3_binary"]])
    want = np.stack([z["out_3_noise_lanczos"], z["out_3_binary_lanczos"]])
    src = dev(batch)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for wide in (0, 1):      # wide = 1: the header sends the kernels down the 32-bit multiply; the same bytes
        ht, vt = host_table(lib, W, out_w, 1), host_table(lib, H, out_h, 1)
        assert ht[1] == 0 and vt[1] == 0
        ht[1] = vt[1] = wide
        dh, dv = dev(ht), dev(vt)
        for path in (K.TWO_PASS, K.TILED, 0):
            for win in (None, (3, 4, 9, 11)):
                r0, c0, h, w = win if win else (0, 0, out_h, out_w)
                cwin = (ctypes.c_int * 4)(*win) if win else None
                nws = lib.sgr_pil_resize_workspace_bytes(2, H, W, 3, out_h, out_w, cwin, 1)
                assert nws > 0
                guard = 64
                ws = torch.full((nws + 2 * guard,), 0xAB, dtype=torch.uint8, device="cuda")
                dst = torch.full((2 * h * w * 3 + 2 * guard,), 0xCD, dtype=torch.uint8, device="cuda")
                rc = lib.sgr_pil_resize_u8(ptr(src), 2, H, W, 3, ctypes.c_void_p(dst.data_ptr() + guard), out_h, out_w, cwin, 1, ptr(dh), ptr(dv),
                                           ctypes.c_void_p(ws.data_ptr() + guard), path, stream)
                assert rc == 0, lib.sgr_last_error()
                torch.cuda.synchronize()
                got = dst[guard:-guard].view(2, h, w, 3).cpu().numpy()
                assert np.array_equal(got, want[:, r0:r0 + h, c0:c0 + w]), (wide, path, win)
                # nothing written around the output or around the workspace
                assert (dst[:guard] == 0xCD).all() and (dst[-guard:] == 0xCD).all() and (ws[:guard] == 0xAB).all() and (ws[-guard:] == 0xAB).all()
    # a single pass and the copy take NULL tables and no workspace
    z = fixture("c4")
    dst = torch.empty(20 * 47 * 3, dtype=torch.uint8, device="cuda")
    dv = dev(host_table(lib, 33, 20, 3))
    assert lib.sgr_pil_resize_u8(ptr(dev(z["im_3_smooth"])), 1, 33, 47, 3, ptr(dst), 20, 47, None, 3, None, ptr(dv), None, 0, stream) == 0, lib.sgr_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(dst.view(20, 47, 3).cpu().numpy(), z["out_3_smooth_bicubic"])
    z = fixture("c10")
    dst = torch.empty(33 * 47 * 3, dtype=torch.uint8, device="cuda")
    assert lib.sgr_pil_resize_u8(ptr(dev(z["im_3_smooth"])), 1, 33, 47, 3, ptr(dst), 33, 47, None, 1, None, None, None, 0, stream) == 0, lib.sgr_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(dst.view(33, 47, 3).cpu().numpy(), z["im_3_smooth"]) and np.array_equal(z["im_3_smooth"], z["out_3_smooth_lanczos"])


# ---- HIP graph ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["two_pass", "tiled"])
def test_graph_capture_and_replay_after_a_warm_up_call(sgr, path):
    z = fixture("c2")
    static = dev(np.stack([z["im_3_noise"], z["im_3_smooth"]]))
    step = lambda: sgr.pil_resize(static, (20, 17), window=(1, 2, 15, 17), path=path)
    eager = step().clone()      # the warm-up call: builds the geometry's tables and copies them to the device
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):      # torch's capture recipe: first uses (allocator growth) on a side stream
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static.copy_(dev(np.stack([z["im_3_binary"], z["im_3_noise"]])))      # new bytes in place: the replay resizes them
    g.replay()
    torch.cuda.synchronize()
    want = np.stack([z["out_3_binary_lanczos"], z["out_3_noise_lanczos"]])[:, 1:16, 2:19]
    assert same(out, want) and not torch.equal(out, eager)


# ---- the loaders' compositions --------------------------------------------------------------------------------------------------------------

def test_iiw_resize_crop_then_iiw_image(sgr):
    z = fixture("c13_C3_noise")
    photo, full = dev(z["im_3_noise"]), z["out_3_noise_lanczos"]
    for cs in K.IIW_CS:
        crop, newH, newW, rs, c = sgr.iiw_resize_crop(photo, 240, 320, cs)
        assert (newH, newW, rs, c) == (240, 361, 0, cs) and same(crop, full[:, cs:cs + 320])
        got = sgr.iiw_image(crop[None])
        pil = full[None, :, cs:cs + 320]      # iiwDataLoader.py:136-137, 205-214 on PIL's bytes, by the loaders' checker
        w32, w64 = RK.iiw_image(pil, np.float32), RK.iiw_image(pil, np.float64)
        assert RK.rel_l2(got.cpu().numpy(), w64) <= RK.bound_of(RK.rel_l2(w32, w64)) and torch.equal(got, sgr.iiw_image(dev(pil)))
    # a portrait photograph: the crop moves along the rows
    tall = dev(np.ascontiguousarray(z["im_3_noise"].transpose(1, 0, 2)[:, :171]))
    crop, newH, newW, rs, c = sgr.iiw_resize_crop(tall, 24, 32, 40)
    want = K.resize(tall.cpu().numpy(), (newW, newH), "lanczos", (40, 0, 24, 32))
    assert (newH, newW, rs, c) == K.iiw_geometry(512, 171, 24, 32)[:2] + (40, 0) and same(crop, want)


def test_loader_resize_then_prepare_batch(sgr):
    z = fixture("c1")      # 48 x 64 "PNGs" to 24 x 32
    full = dict(seg=z["im_3_binary"], albedo=z["im_3_noise"], normal=z["im_3_smooth"], rough=z["im_1_noise"])
    pil = dict(seg=z["out_3_binary_lanczos"], albedo=z["out_3_noise_lanczos"], normal=z["out_3_smooth_lanczos"], rough=z["out_1_noise_lanczos"])
    rng = np.random.default_rng(311)
    rest = dict(im=(rng.random((2, 24, 32, 3)) ** 2 * 4).astype(np.float32), depth=(rng.random((2, 24, 32)) * 5 + 1).astype(np.float32))
    batch_of = lambda d: {k: np.stack([v, v[::-1].copy() if v.shape[0] == 48 else v[:, ::-1].copy()]) for k, v in d.items()}
    raw_full, raw_pil = batch_of(full), {k: np.stack([pil[k], K.resize(batch_of(full)[k][1], (32, 24))]) for k in pil}
    raw = sgr.loader_resize({**{k: dev(v) for k, v in raw_full.items()}, **{k: dev(v) for k, v in rest.items()}, "name": ["a", "b"]}, (32, 24))
    for k in pil:
        assert same(raw[k], raw_pil[k]), k
    got = sgr.prepare_batch(raw, "TEST", False)
    ref = sgr.prepare_batch({**{k: dev(v) for k, v in raw_pil.items()}, **{k: dev(v) for k, v in rest.items()}, "name": ["a", "b"]}, "TEST", False)
    assert sorted(got) == sorted(ref) and got["name"] == ["a", "b"]
    for k in ref:
        if k != "name":
            assert torch.equal(got[k], ref[k]), k
    # dataLoader.py:139-147 and :120-131 on PIL's bytes, by the loader's checker
    host = {**raw_pil, **rest}
    c32, c64 = LK.prepare_batch(host, "TEST", False, None, dtype=np.float32), LK.prepare_batch(host, "TEST", False, None, dtype=np.float64)
    for k in ("albedo", "normal", "rough"):
        assert LK.rel(got[k].cpu().numpy(), c64[k]) <= max(2.0 * LK.rel(c32[k], c64[k]), 1e-6), k
    for k in ("segArea", "segEnv", "segObj"):
        assert np.array_equal(got[k].cpu().numpy(), c64[k]), k
