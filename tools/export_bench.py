"""Times of the export operators (sgr.export_*) on one photograph's worth of testReal outputs: 240 x 320 predictions written at 480 x 640
(albedo with its cAlbedo, normal, rough, depth, rendered; the shading at 120 x 160) and one [1,3,120,160,8,16] env image (the .npz layout
and the nrows=24, ncols=16 mosaic).

    python tools/export_bench.py [--reps 80] [--warmup 5] [--out FILE.json] [--no-host]
    rocprofv3 --kernel-trace --stats ... -- python tools/export_bench.py --profile     # the fused calls only, few repetitions

Candidates, alternating in one process, device events around each call, the median of >= 80 with the min-max spread:

  fused    the operators: the six images, the two env calls
  eager    the same arithmetic as PyTorch-ROCm expressions on the same device tensors (F.interpolate's bilinear rule stands in for OpenCV's;
           permute / flip / contiguous for the env copy; a strided slice, pad and permute for the mosaic)

and, in columns of their own:

  host     the reference's route, wall clock, best of 5: the fp32 tensors copied to the host with .cpu(), then the numpy lines of
           testReal.py:542-657 and utils.writeEnvToFile, torch's CPU bilinear standing in for cv2.resize (not installed); no file is encoded
  d2h      device -> pinned host of the fused results beside that of the fp32 tensors they are made from
  floor    bytes read + written, from shapes, at 8 TB/s, as a share of the call's time: the albedo image and export_env_hwc"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 8.0
H, W, NH, NW, R, C, EH, EW = 240, 320, 480, 640, 120, 160, 8, 16
G = 1.0 / 2.2


def u8(t):
    return t.clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).flip(-1).contiguous()


def up(x):
    return F.interpolate(x, size=(NH, NW), mode="bilinear", align_corners=False)


def eager_images(p, c_albedo):
    d = p["depth"] / p["depth"].mean().clamp_min(1e-10) * 3
    return dict(albedo=u8(255 * up((p["albedo"] * c_albedo) ** G)), normal=u8(255 * 0.5 * (up(p["normal"]) + 1)), rough=u8(255 * 0.5 * (up(p["rough"]) + 1)),
                depth=u8(255 * (1 / (up(d) + 1).clamp(1e-6, 10))), rendered=u8(up((p["rendered"] / p["rendered"].max()) ** G).clamp(0, 1) * 255),
                shading=u8(255 * (p["shading"] / p["shading"].mean() / 3).clamp(0, 1) ** G))


def eager_env_hwc(env):
    return env.permute(0, 2, 3, 4, 5, 1).flip(-1).contiguous()


def eager_mosaic(env, nrows=24, ncols=16, gap=1):
    cells = env[:, :, ::R // nrows, ::C // ncols]                                      # [B,3,ty,tx,eh,ew]
    cells = F.pad(cells.clamp(0, 1) ** G, (0, gap, 0, gap), value=1.0)
    B, _, ty, tx, ph, pw = cells.shape
    big = cells.permute(0, 2, 4, 3, 5, 1).reshape(B, ty * ph, tx * pw, 3)
    big = F.pad(big, (0, 0, 0, gap, 0, gap), value=1.0)                                # the closing margin
    return (255 * big).to(torch.uint8).flip(-1).contiguous()


def host_route(p, env, c_albedo):
    """the reference's lines on the host; returns nothing: only the time matters"""
    rs = lambda a: F.interpolate(torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1) if a.ndim == 3 else a[None]))[None], size=(NH, NW), mode="bilinear",
                                 align_corners=False)[0].numpy().transpose(1, 2, 0)
    a = (p["albedo"] * c_albedo).data.cpu().numpy().squeeze().transpose([1, 2, 0]) ** (1.0 / 2.2)
    out = [np.clip(255 * rs(a), 0, 255).astype(np.uint8)[:, :, ::-1]]
    n = rs(p["normal"].data.cpu().numpy().squeeze().transpose([1, 2, 0]))
    out.append((255 * 0.5 * (n + 1)).astype(np.uint8)[:, :, ::-1])
    out.append((255 * 0.5 * (rs(p["rough"].data.cpu().numpy().squeeze()) + 1)).astype(np.uint8))
    d = p["depth"].data.cpu().numpy().squeeze()
    d = rs(d / np.maximum(d.mean(), 1e-10) * 3)
    out.append((255 * (1 / np.clip(d + 1, 1e-6, 10))).astype(np.uint8))
    r = p["rendered"].data.cpu().numpy().squeeze().transpose([1, 2, 0])
    out.append((np.clip(rs((r / r.max()) ** (1.0 / 2.2)), 0, 1) * 255).astype(np.uint8)[:, :, ::-1])
    s = p["shading"].data.cpu().numpy().squeeze().transpose([1, 2, 0])
    out.append((255 * np.clip(s / np.mean(s) / 3.0, 0, 1) ** (1.0 / 2.2)).astype(np.uint8)[:, :, ::-1])
    e = env.data.cpu().numpy().squeeze().transpose([1, 2, 3, 4, 0])
    out.append(np.ascontiguousarray(e[:, :, :, :, ::-1]))
    iy, ix = R // 24, C // 16
    big = np.zeros([24 * (EH + 1) + 1, 16 * (EW + 1) + 1, 3], dtype=np.float32) + 1.0
    for r_ in range(0, R, iy):
        for c_ in range(0, C, ix):
            rs_, cs_ = (r_ // iy) * (EH + 1), (c_ // ix) * (EW + 1)
            big[rs_:rs_ + EH, cs_:cs_ + EW, :] = e[r_, c_]
    out.append((255 * (np.clip(big, 0, 1) ** (1.0 / 2.2))).astype(np.uint8)[:, :, ::-1])
    return out


def timed(fns, reps, warm):
    """{name: sorted ms} for the callables, alternating inside every repetition"""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1))
    return {k: sorted(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import inverserenderingofindoorscene_amd as sgr
    if not torch.cuda.is_available():
        raise SystemExit("export_bench needs a GPU")
    reps, warm = (3, 1) if args.profile else (max(80, args.reps), args.warmup)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g)
    p = dict(albedo=rnd(1, 3, H, W), normal=2 * rnd(1, 3, H, W) - 1, rough=2 * rnd(1, 1, H, W) - 1, depth=0.2 + 4 * rnd(1, 1, H, W), rendered=rnd(1, 3, H, W) ** 2 * 3,
             shading=rnd(1, 3, R, C) ** 2 * 2)
    p = {k: v.cuda() for k, v in p.items()}
    env = (1.2 * rnd(1, 3, R, C, EH, EW)).cuda()
    c_albedo = 0.8
    scale = torch.tensor([c_albedo], device="cuda")

    def fused_images():
        return dict(albedo=sgr.export_image(p["albedo"], "albedo", (NH, NW), scale, True), normal=sgr.export_image(p["normal"], "normal", (NH, NW), None, True),
                    rough=sgr.export_image(p["rough"], "rough", (NH, NW)), depth=sgr.export_image(p["depth"], "depth", (NH, NW)),
                    rendered=sgr.export_image(p["rendered"], "rendered", (NH, NW), None, True), shading=sgr.export_image(p["shading"], "shading", None, None, True))

    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "shape": dict(h=H, w=W, nh=NH, nw=NW, R=R, C=C, eh=EH, ew=EW), "ms": {}}
    with torch.no_grad():      # the two forms agree before they are timed (another resize rule and pow: a byte may differ by one, rarely more at an edge)
        a, b = fused_images(), eager_images(p, c_albedo)
        rec["largest_byte_difference_fused_vs_eager"] = {k: int((a[k].int() - b[k].int()).abs().max()) for k in a}
        rec["share_of_bytes_that_differ_fused_vs_eager"] = {k: float((a[k] != b[k]).float().mean()) for k in a}
        assert torch.equal(sgr.export_env_hwc(env), eager_env_hwc(env))
        m1, m2 = sgr.export_env_mosaic(env, 24, 16, bgr=True), eager_mosaic(env)
        assert m1.shape == m2.shape and int((m1.int() - m2.int()).abs().max()) <= 1
        print("fused vs eager, largest byte difference:", rec["largest_byte_difference_fused_vs_eager"])

    fns = {"fused_images": fused_images, "fused_albedo": lambda: sgr.export_image(p["albedo"], "albedo", (NH, NW), scale, True),
           "fused_env_hwc": lambda: sgr.export_env_hwc(env), "fused_env_mosaic": lambda: sgr.export_env_mosaic(env, 24, 16, bgr=True)}
    if not args.profile:
        fns.update({"eager_images": lambda: eager_images(p, c_albedo), "eager_albedo": lambda: u8(255 * up((p["albedo"] * c_albedo) ** G)),
                    "eager_env_hwc": lambda: eager_env_hwc(env), "eager_env_mosaic": lambda: eager_mosaic(env)})
        res = fused_images()
        res.update(hwc=sgr.export_env_hwc(env), mosaic=sgr.export_env_mosaic(env, 24, 16, bgr=True))
        src = dict(p, env=env)
        pin = lambda d: {k: torch.empty(v.shape, dtype=v.dtype).pin_memory() for k, v in d.items()}
        pin_res, pin_src = pin(res), pin(src)
        pin_img, pin_img_src = {k: v for k, v in pin_res.items() if k not in ("hwc", "mosaic")}, {k: v for k, v in pin_src.items() if k != "env"}
        copy = lambda dst, frm: [dst[k].copy_(frm[k], non_blocking=True) for k in dst]
        fns["d2h_fused_images"] = lambda: copy(pin_img, res)
        fns["d2h_fp32_images"] = lambda: copy(pin_img_src, src)
        fns["d2h_fused_mosaic"] = lambda: pin_res["mosaic"].copy_(res["mosaic"], non_blocking=True)
        fns["d2h_fp32_env"] = lambda: pin_src["env"].copy_(env, non_blocking=True)      # also what the .npz copy costs, fused or not: the same bytes
        rec["d2h_bytes"] = dict(fused_images=sum(v.numel() for v in pin_img.values()), fp32_images=4 * sum(v.numel() for v in pin_img_src.values()),
                                fused_mosaic=res["mosaic"].numel(), fp32_env=4 * env.numel())
    with torch.no_grad():
        t = timed(fns, reps, warm)
    for name, v in t.items():
        med = statistics.median(v)
        rec["ms"][name] = dict(median=med, min=v[0], max=v[-1])
        print(f"{name:22s} median {med * 1e3:10.1f} us  min {v[0] * 1e3:10.1f}  max {v[-1] * 1e3:10.1f}")
    floors = dict(fused_albedo=4 * 3 * H * W + 3 * NH * NW, fused_env_hwc=2 * 4 * env.numel())
    rec["byte_floor"] = {}
    for name, nbytes in floors.items():
        us = nbytes / (HBM_TBPS * 1e12) * 1e6
        share = us / (rec["ms"][name]["median"] * 1e3)
        rec["byte_floor"][name] = dict(bytes=nbytes, floor_us_at_8TBps=us, share_of_call_time=share)
        print(f"{name:22s} {nbytes} bytes: floor {us:.2f} us at {HBM_TBPS} TB/s, share of the call's time {share:.3f}")
    if not args.profile:
        for op in ("images", "albedo", "env_hwc", "env_mosaic"):
            f_, e_ = rec["ms"]["fused_" + op], rec["ms"]["eager_" + op]
            overlap = f_["max"] >= e_["min"] and e_["max"] >= f_["min"]
            rec["ms"][op + "_eager_over_fused"] = dict(ratio=e_["median"] / f_["median"], spreads_overlap=overlap, fused_slower=f_["median"] > e_["median"])
            print(f"{op:22s} eager / fused = {e_['median'] / f_['median']:.2f}x" + ("  SPREADS OVERLAP" if overlap else "") + ("  FUSED SLOWER" if f_["median"] > e_["median"] else ""))
    if not (args.profile or args.no_host):
        best = None
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_route(p, env, c_albedo)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        rec["host_route_ms_best_of_5"] = best * 1e3
        def device_route():
            r_ = fused_images()
            r_.update(hwc=sgr.export_env_hwc(env), mosaic=sgr.export_env_mosaic(env, 24, 16, bgr=True))
            return [v.cpu() for v in r_.values()]
        bd = None
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device_route()
            dt = time.perf_counter() - t0
            bd = dt if bd is None else min(bd, dt)
        rec["device_route_ms_best_of_5"] = bd * 1e3
        print(f"host route (fp32 .cpu() + numpy, torch CPU bilinear for cv2): {best * 1e3:.1f} ms; fused calls + .cpu() of the results: {bd * 1e3:.1f} ms (wall clock, best of 5)"
              + ("  DEVICE ROUTE SLOWER" if bd > best else ""))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
