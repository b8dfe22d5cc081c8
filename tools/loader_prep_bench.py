"""Times of the loader-preparation operators (sgr.loader_* / sgr.prepare_batch) at the training size: batch 16, 240 x 320 planes, a 120 x 160
grid of 16 x 32 env cells reduced to 8 x 16.

    python tools/loader_prep_bench.py [--reps 80] [--warmup 5] [--out FILE.json] [--no-host]
    rocprofv3 --kernel-trace --stats ... -- python tools/loader_prep_bench.py --profile     # the fused calls only, few repetitions

Candidates, alternating in one process, device events around each call, the median of >= 80 with the min-max spread:

  fused    the operators, one by one and as prepare_batch
  eager    a PyTorch-ROCm composition on the same device tensors: reshape / permute / contiguous / mean for the env map, sort for the order
           statistic, max_pool2d for the erosion, point-wise expressions for the maps

and, in columns of their own, what decides whether moving the arithmetic is worth the 4x larger upload:

  copy     pinned host -> device of the raw batch (16 x 32 cells) beside the copy of the reduced batch (8 x 16) the reference's loader hands over
  host     the reference's numpy composition for the env map (reshape / transpose / ascontiguousarray / block mean) over the batch with 16
           threads, wall clock, best of 3

The byte floor of the env map is 4 * 3 * bn * R * C * (16 * 32 + eh * ew) bytes at 8 TB/s."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 8.0
BN, H, W, R, C, EH, EW = 16, 240, 320, 120, 160, 8, 16


def eager_env(raw, scale):
    bn = raw.shape[0]
    e = raw.view(bn, R, 16, C, 32, 3).permute(0, 5, 1, 3, 2, 4).contiguous()
    return e.view(bn, 3, R, C, EH, 2, EW, 2).mean((5, 7)) * scale.view(bn, 1, 1, 1, 1, 1)


def eager_seg(seg_u8):
    return 0.5 * ((seg_u8[..., 0].float() - 127.5) / 127.5 + 1)


def eager_masks(seg_u8):
    seg = eager_seg(seg_u8).unsqueeze(1)
    area, env, obj = ((seg > 0.49) & (seg < 0.51)).float(), (seg < 0.1).float(), (seg > 0.9).float()
    return area, env, 1.0 - F.max_pool2d(1.0 - obj, 7, stride=1, padding=3)


def eager_scale_hdr(hdr, seg_u8, num, k):
    prod = (hdr * eager_seg(seg_u8).unsqueeze(-1)).flatten(1)
    v = prod.sort(dim=1).values[:, k]
    scale = num / v.clamp_min(0.1)
    return (scale.view(-1, 1, 1, 1) * hdr).clamp(0, 1).permute(0, 3, 1, 2).flip(1).contiguous(), scale


def eager_maps(a8, n8, r8):
    chw = lambda x: ((x.float() - 127.5) / 127.5).permute(0, 3, 1, 2)
    n = chw(n8)
    return (0.5 * (chw(a8) + 1)) ** 2.2, n / (n * n).sum(1, keepdim=True).clamp_min(1e-5).sqrt(), chw(r8)[:, 0:1].contiguous()


def host_env(raw):
    """loadEnvmap's arithmetic (dataLoader.py:301-307) for one image, block_reduce written as the mean over the block axes"""
    env = np.ascontiguousarray(raw.reshape(R, 16, C, 32, 3).transpose([4, 0, 2, 1, 3]))
    return env.reshape(3, R, C, EH, 2, EW, 2).mean(axis=(4, 6))


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
        raise SystemExit("loader_prep_bench needs a GPU")
    reps, warm = (3, 1) if args.profile else (max(80, args.reps), args.warmup)
    g = torch.Generator().manual_seed(0)
    q = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)
    seg = torch.where(torch.rand(BN, H, W, 3, generator=g) < 0.6, torch.tensor(255, dtype=torch.uint8), q(BN, H, W, 3))
    host = dict(seg=seg, im=torch.rand(BN, H, W, 3, generator=g) ** 3 * 6, albedo=q(BN, H, W, 3), normal=q(BN, H, W, 3), rough=q(BN, H, W, 3),
                depth=torch.rand(BN, H, W, generator=g), envmaps=torch.rand(BN, R * 16, C * 32, 3, generator=g), envmapsInd=torch.ones(BN))
    d = {k: v.cuda() for k, v in host.items()}
    u = torch.rand(BN, generator=g).cuda()
    num = (0.95 - 0.1 * u.double()).float()
    k = int(0.95 * W * H * 3)
    scale = sgr.loader_scale_hdr(d["im"], d["seg"], u)[1]
    env_bytes = 4 * 3 * BN * R * C * (16 * 32 + EH * EW)
    floor_us = env_bytes / (HBM_TBPS * 1e12) * 1e6
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "shape": dict(bn=BN, H=H, W=W, R=R, C=C, eh=EH, ew=EW), "ms": {},
           "env_bytes": env_bytes, "env_floor_us_at_8TBps": floor_us}

    with torch.no_grad():      # the two forms agree before they are timed
        a, b = sgr.loader_envmaps(d["envmaps"], scale), eager_env(d["envmaps"], scale)
        rec["env_rel_l2_fused_vs_eager"] = float((a.double() - b.double()).norm() / b.double().norm())
        assert torch.equal(sgr.loader_masks(d["seg"])[2], eager_masks(d["seg"])[2])
        torch.testing.assert_close(sgr.loader_scale_hdr(d["im"], d["seg"], u)[1], eager_scale_hdr(d["im"], d["seg"], num, k)[1], rtol=1e-6, atol=0)
        del a, b

    fns = {"fused_envmaps": lambda: sgr.loader_envmaps(d["envmaps"], scale), "fused_scale_hdr": lambda: sgr.loader_scale_hdr(d["im"], d["seg"], u),
           "fused_masks": lambda: sgr.loader_masks(d["seg"]), "fused_brdf_maps": lambda: sgr.loader_brdf_maps(d["albedo"], d["normal"], d["rough"]),
           "fused_prepare_batch": lambda: sgr.prepare_batch(d, "TRAIN", True, u)}
    if not args.profile:
        with torch.no_grad():
            fns.update({"eager_envmaps": lambda: eager_env(d["envmaps"], scale), "eager_scale_hdr": lambda: eager_scale_hdr(d["im"], d["seg"], num, k),
                        "eager_masks": lambda: eager_masks(d["seg"]), "eager_brdf_maps": lambda: eager_maps(d["albedo"], d["normal"], d["rough"])})
        pin_raw = host["envmaps"].pin_memory()
        pin_red = torch.empty(BN, 3, R, C, EH, EW).pin_memory()
        dst_red = torch.empty(BN, 3, R, C, EH, EW, device="cuda")
        fns["copy_raw_batch"] = lambda: d["envmaps"].copy_(pin_raw, non_blocking=True)
        fns["copy_reduced_batch"] = lambda: dst_red.copy_(pin_red, non_blocking=True)
    with torch.no_grad():
        t = timed(fns, reps, warm)
    for name, v in t.items():
        med = statistics.median(v)
        rec["ms"][name] = dict(median=med, min=v[0], max=v[-1])
        note = f"  byte floor {floor_us:.0f} us at {HBM_TBPS} TB/s: share {floor_us / (med * 1e3):.2f}" if name == "fused_envmaps" else ""
        print(f"{name:22s} median {med * 1e3:10.1f} us  min {v[0] * 1e3:10.1f}  max {v[-1] * 1e3:10.1f}{note}")
    rec["env_share_of_floor"] = floor_us / (rec["ms"]["fused_envmaps"]["median"] * 1e3)
    if not args.profile:
        for op in ("envmaps", "scale_hdr", "masks", "brdf_maps"):
            f_, e_ = rec["ms"]["fused_" + op], rec["ms"]["eager_" + op]
            overlap = f_["max"] >= e_["min"]
            rec["ms"][op + "_eager_over_fused"] = dict(ratio=e_["median"] / f_["median"], spreads_overlap=overlap, fused_slower=f_["median"] > e_["median"])
            print(f"{op:22s} eager / fused = {e_['median'] / f_['median']:.2f}x" + ("  SPREADS OVERLAP" if overlap else "") + ("  FUSED SLOWER" if f_["median"] > e_["median"] else ""))
        extra = rec["ms"]["copy_raw_batch"]["median"] - rec["ms"]["copy_reduced_batch"]["median"]
        rec["extra_upload_ms"] = extra
        print(f"extra upload of the raw batch: {extra:.2f} ms per batch; fused env map {rec['ms']['fused_envmaps']['median']:.3f} ms")
    if not (args.profile or args.no_host):
        raws = [host["envmaps"][b].numpy() for b in range(BN)]
        best = None
        with ThreadPoolExecutor(16) as pool:
            for _ in range(3):
                t0 = time.perf_counter()
                list(pool.map(host_env, raws))
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
        rec["host_numpy_env_16_threads_ms"] = best * 1e3
        total = rec["ms"]["fused_envmaps"]["median"] + rec["extra_upload_ms"]
        rec["device_route_slower_than_host"] = total > best * 1e3
        print(f"host numpy env map, 16 threads, batch of {BN}: {best * 1e3:.1f} ms (best of 3); fused + extra upload {total:.2f} ms" + ("  DEVICE ROUTE SLOWER" if total > best * 1e3 else ""))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
