"""Times of the real-image loader operators (sgr.nyu_prepare_batch, sgr.iiw_image) at the fine-tuning sizes: batch 16, source 480 x 640, TRAIN
crops (560..600 wide) to 240 x 320 (trainFineTuneNYU.py's default) and to 480 x 640; IIW images of 240 x 320.

    python tools/real_loader_prep_bench.py [--reps 80] [--warmup 5] [--out FILE.json] [--no-host]
    python tools/real_loader_prep_bench.py --step nyu240          # one step in this process

Without --step the tool never touches the GPU itself: every step runs in a fresh child process under a time limit of its own, one after the
other, and the first step that fails, faults or runs out of time ends the run (nothing more is started on the device).

Steps and candidates (inside a step they alternate in one process, device events around each call, the median of >= 80 with the min-max
spread):

  stream         a device-to-device copy of 512 MiB: the HBM rate a plain streaming kernel reaches here (read + write bytes over the time)
  nyu240 nyu480  fused_direct / fused_staged: sgr.nyu_prepare_batch with the kernel's two forms (SGR_NYU_STAGE=0 / 1), the crop / flip / colour
                 tensors on the device; eager: a PyTorch-ROCm composition on the same device tensors -- a per-image crop, F.interpolate(bilinear)
                 and point-wise operators: the same work, though torch's rule and not OpenCV's
  iiw            sgr.iiw_image against (x.float() / 255) ** 2.2, permute, a division by amax
  copy           pinned host -> device of the raw batch (three uint8 HWC images and the fp32 depth: 13 bytes per source pixel) beside the copy
                 of the prepared batch (nine fp32 planes: 36 bytes per output pixel) the reference's loader hands over
  host           the checker's fp32 numpy composition (tests/real_loader_checker.py: the reference's own order of operations) over the batch
                 with 16 threads, wall clock, best of 3

The byte floor of nyu_prepare is 13 bytes per pixel of the crops + 36 bytes per output pixel, of iiw_image 2 * 3 + 12 bytes per pixel, at the
rate the `stream` step measured (the share at the 8 TB/s of the data sheet is printed beside it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBPS = 8.0
BN, HS, WS = 16, 480, 640
STEPS = (("stream", 120), ("nyu240", 240), ("nyu480", 240), ("iiw", 120), ("copy", 180), ("host", 300))      # (step, its time limit in seconds)


def timed(fns, reps, warm):
    """{name: sorted ms} for the callables, alternating inside every repetition"""
    import torch
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


def summary(t):
    return {k: dict(median=statistics.median(v), min=v[0], max=v[-1]) for k, v in t.items()}


def raw_batch(seed=0):
    import real_loader_checker as K
    return K.draw_raw(BN, HS, WS, seed)


def eager_nyu(d, crops, flip, colour, H, W):
    """the same work in eager PyTorch: torch's bilinear rule, not OpenCV's"""
    import torch
    import torch.nn.functional as F
    outs = []
    for b, (rs, cs, ch, cw) in enumerate(crops):
        chw = lambda x: x[b, rs:rs + ch, cs:cs + cw].flip(-1).permute(2, 0, 1).float()
        im = 0.5 * ((2 * (chw(d["im"]) / 255.0) ** 2.2 - 1) + 1)
        n = (chw(d["normal"]) - 127.5) / 127.5
        n = n / (n * n).sum(0, keepdim=True).clamp_min(1e-5).sqrt()
        sn = 0.5 * ((chw(d["seg"])[0:1] - 127.5) / 127.5 + 1)
        x = torch.cat([n, d["depth"][b:b + 1, rs:rs + ch, cs:cs + cw], sn, im], 0)[None]
        if (ch, cw) != (H, W):
            x = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
        outs.append(x)
    x = torch.cat(outs, 0)
    n, dep, sn, im = x[:, 0:3], x[:, 3:4], x[:, 4:5], x[:, 5:8]
    sd = ((dep > 1) & (dep < 10)).float()
    n = n / (n * n).sum(1, keepdim=True).sqrt().clamp_min(1e-5)
    f = flip.view(-1, 1, 1, 1)
    mirror = lambda v: torch.where(f, v.flip(-1), v)
    n = mirror(n) * torch.where(f, torch.tensor([-1.0, 1.0, 1.0], device=n.device).view(1, 3, 1, 1), torch.ones(1, 3, 1, 1, device=n.device))
    return n, mirror(dep), mirror(sn), mirror(sd), (mirror(im).double() * colour.view(-1, 3, 1, 1)).float()


def step_stream(args):
    import torch
    x = torch.empty(512 << 20, dtype=torch.uint8, device="cuda").random_()
    y = torch.empty_like(x)
    t = summary(timed({"d2d_copy_512MiB": lambda: y.copy_(x)}, args.reps, args.warmup))
    rate = 2 * x.numel() / (t["d2d_copy_512MiB"]["median"] * 1e-3) / 1e12
    print(f"stream: device-to-device copy of 512 MiB, median {t['d2d_copy_512MiB']['median'] * 1e3:.1f} us: {rate:.2f} TB/s (read + write)")
    return dict(ms=t, stream_tbps=rate)


def step_nyu(args, H, W):
    import torch
    import inverserenderingofindoorscene_amd as sgr
    import real_loader_checker as K
    raw = raw_batch()
    d = {k: torch.from_numpy(v).cuda() for k, v in raw.items()}
    u = torch.from_numpy(np.random.default_rng(1).random((BN, 7)))
    crop, flip, colour = sgr.nyu_augmentation(u.cuda(), H, W)
    crops = [tuple(int(v) for v in row) for row in crop.cpu().tolist()]
    floor_bytes = sum(13 * ch * cw for _, _, ch, cw in crops) + 36 * BN * H * W

    def fused(stage):
        def f():
            os.environ["SGR_NYU_STAGE"] = stage
            return sgr.nyu_prepare_batch(d, "TRAIN", crop, flip, colour, imHeight=H, imWidth=W)
        return f
    with torch.no_grad():      # the forms agree before they are timed
        a, b = fused("0")(), fused("1")()
        assert all(torch.equal(a[k], b[k]) for k in K.NYU_KEYS)
        e = eager_nyu(d, crops, flip, colour, H, W)
        rel = {k: float((a[k].double() - v.double()).norm() / v.double().norm()) for k, v in zip(("normal", "depth", "segNormal", "segDepth", "im"), e)}
        want = K.nyu_sample(raw["im"][3], raw["normal"][3], raw["seg"][3], raw["depth"][3], crops[3], bool(flip[3]), colour[3].cpu().numpy(), H, W, np.float64)
        rel64 = {k: K.rel_l2(a[k][3].cpu().numpy(), want[k]) for k in ("normal", "depth", "segNormal", "im")}
        assert max(rel64.values()) < 1e-6, rel64
        fns = {"fused_direct": fused("0"), "fused_staged": fused("1"), "eager": lambda: eager_nyu(d, crops, flip, colour, H, W)}
        t = summary(timed(fns, args.reps, args.warmup))
    rec = dict(ms=t, shape=dict(bn=BN, Hs=HS, Ws=WS, H=H, W=W, crops=crops), floor_bytes=floor_bytes, rel_l2_fused_vs_eager_torch_rule=rel, rel_l2_fused_vs_fp64_checker_image3=rel64)
    for k, v in t.items():
        print(f"nyu {H}x{W} {k:14s} median {v['median'] * 1e3:9.1f} us  min {v['min'] * 1e3:9.1f}  max {v['max'] * 1e3:9.1f}")
    for k in ("fused_staged", "eager"):
        overlap = t["fused_direct"]["max"] >= t[k]["min"] and t[k]["max"] >= t["fused_direct"]["min"]
        rec[k + "_over_fused_direct"] = dict(ratio=t[k]["median"] / t["fused_direct"]["median"], spreads_overlap=overlap)
        print(f"nyu {H}x{W} {k} / fused_direct = {t[k]['median'] / t['fused_direct']['median']:.2f}x" + ("  SPREADS OVERLAP" if overlap else ""))
    print(f"nyu {H}x{W} byte floor: {floor_bytes / 1e6:.1f} MB = {floor_bytes / (HBM_TBPS * 1e12) * 1e6:.1f} us at {HBM_TBPS} TB/s")
    return rec


def step_iiw(args):
    import torch
    import inverserenderingofindoorscene_amd as sgr
    H, W = 240, 320
    im = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (BN, H, W, 3), dtype=np.uint8)).cuda()

    def eager():
        x = ((im.float() / 255.0) ** 2.2).permute(0, 3, 1, 2)
        return x / x.amax((1, 2, 3), keepdim=True)
    with torch.no_grad():
        a, b = sgr.iiw_image(im), eager()
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        assert rel < 1e-6, rel
        t = summary(timed({"fused": lambda: sgr.iiw_image(im), "eager": eager}, args.reps, args.warmup))
    floor_bytes = BN * H * W * (2 * 3 + 12)
    for k, v in t.items():
        print(f"iiw {H}x{W} {k:14s} median {v['median'] * 1e3:9.1f} us  min {v['min'] * 1e3:9.1f}  max {v['max'] * 1e3:9.1f}")
    overlap = t["fused"]["max"] >= t["eager"]["min"]
    print(f"iiw eager / fused = {t['eager']['median'] / t['fused']['median']:.2f}x" + ("  SPREADS OVERLAP" if overlap else "") + ("  FUSED SLOWER" if t["fused"]["median"] > t["eager"]["median"] else ""))
    return dict(ms=t, shape=dict(bn=BN, H=H, W=W), floor_bytes=floor_bytes, rel_l2_fused_vs_eager=rel, eager_over_fused=dict(ratio=t["eager"]["median"] / t["fused"]["median"], spreads_overlap=overlap))


def step_copy(args):
    import torch
    raw = {k: torch.from_numpy(v).pin_memory() for k, v in raw_batch().items()}
    dst = {k: torch.empty_like(v, device="cuda") for k, v in raw.items()}
    fns = {"copy_raw_batch": lambda: [dst[k].copy_(raw[k], non_blocking=True) for k in raw]}
    for H, W in ((240, 320), (480, 640)):
        shapes = ((BN, 3, H, W), (BN, 1, H, W), (BN, 1, H, W), (BN, 1, H, W), (BN, 3, H, W))
        pin = [torch.zeros(s).pin_memory() for s in shapes]
        out = [torch.empty(s, device="cuda") for s in shapes]
        fns[f"copy_prepared_batch_{H}x{W}"] = lambda pin=pin, out=out: [o.copy_(p, non_blocking=True) for o, p in zip(out, pin)]
    t = summary(timed(fns, args.reps, args.warmup))
    rec = dict(ms=t, raw_bytes=13 * BN * HS * WS, prepared_bytes={f"{H}x{W}": 36 * BN * H * W for H, W in ((240, 320), (480, 640))})
    for k, v in t.items():
        print(f"{k:30s} median {v['median']:8.3f} ms  min {v['min']:8.3f}  max {v['max']:8.3f}")
    return rec


def step_host(args):
    import real_loader_checker as K
    raw = raw_batch()
    rec = {}
    for H, W in ((240, 320), (480, 640)):
        rng = np.random.default_rng(1)
        aug = [K.nyu_augmentation(rng.random(7), H, W) for _ in range(BN)]
        one = lambda b: K.nyu_sample(raw["im"][b], raw["normal"][b], raw["seg"][b], raw["depth"][b], aug[b][0], aug[b][1], aug[b][2], H, W, np.float32)
        best = None
        with ThreadPoolExecutor(16) as pool:
            for _ in range(3):
                t0 = time.perf_counter()
                list(pool.map(one, range(BN)))
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
        rec[f"host_numpy_16_threads_ms_{H}x{W}"] = best * 1e3
        print(f"host numpy composition, 16 threads, batch of {BN}, to {H}x{W}: {best * 1e3:.1f} ms (best of 3)")
    return rec


def run_step(args):
    import torch
    if args.step != "host" and not torch.cuda.is_available():
        raise SystemExit("real_loader_prep_bench needs a GPU")
    rec = {"stream": step_stream, "nyu240": lambda a: step_nyu(a, 240, 320), "nyu480": lambda a: step_nyu(a, 480, 640), "iiw": step_iiw, "copy": step_copy, "host": step_host}[args.step](args)
    if args.step != "host":
        rec["device"] = torch.cuda.get_device_name(0)
    print("JSON " + json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", default="", choices=("",) + tuple(s for s, _ in STEPS))
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    args.reps = max(80, args.reps)
    if args.step:
        return run_step(args)
    rec = {"reps": args.reps}
    for step, limit in STEPS:
        if step == "host" and args.no_host:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step} ran past its limit of {limit} s: stopping here")
        lines = r.stdout.splitlines()
        print("\n".join(l for l in lines if not l.startswith("JSON ")), flush=True)
        if r.returncode != 0:
            raise SystemExit(f"step {step} ended with status {r.returncode}: stopping here\n{r.stderr[-3000:]}")
        rec[step] = json.loads([l for l in lines if l.startswith("JSON ")][-1][5:])
    if "stream" in rec:
        rate = rec["stream"]["stream_tbps"]
        for step, key in (("nyu240", "fused_direct"), ("nyu240", "fused_staged"), ("nyu480", "fused_direct"), ("nyu480", "fused_staged"), ("iiw", "fused")):
            if step in rec:
                us = rec[step]["ms"][key]["median"] * 1e3
                floor = rec[step]["floor_bytes"]
                share = dict(of_measured_stream_rate=floor / (rate * 1e12) * 1e6 / us, of_8TBps=floor / (HBM_TBPS * 1e12) * 1e6 / us)
                rec[step].setdefault("share_of_byte_floor", {})[key] = share
                print(f"{step} {key}: {us:.1f} us; byte floor {floor / 1e6:.1f} MB: share {share['of_measured_stream_rate']:.2f} at the measured {rate:.2f} TB/s, {share['of_8TBps']:.2f} at 8 TB/s")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
