"""Times of the bilateral solver layer's operator (sgr.bilateral_solve): forward and forward + backward for modes 0, 2, 4 at 240x320
and 480x640, batch 1 and 4, three target channels for mode 0 and one for modes 2 and 4 (albedo / roughness / depth, testReal.py:534-540).
Each configuration: warm-up, then >= 50 repetitions timed one by one with device events; median, p10, p90.

    python tools/bilateral_bench.py [--reps 60] [--warmup 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/bilateral_bench.py --profile     # one configuration, few repetitions: the per-kernel split

There is no earlier implementation on the GPU to compare with; the reference's CPU times on the machine that made the fixtures are
stored in tests/golden/g13_bilateral_*.npz (``ref_cpu_seconds``) -- another machine, quoted as such."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(B, C, H, W, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    u, v = x / (W - 1), y / (H - 1)
    im = np.stack([np.stack([0.45 + 0.25 * np.sin(2.1 * u + 0.7 * v + p + b) + 0.1 * np.cos(3.3 * v + p) for p in (0.3, 1.1, 2.2)], 0) for b in range(B)])
    im[..., W // 2:] *= 0.7
    im = np.clip(im + 0.0015 * rng.standard_normal(im.shape), 0.05, 0.95).astype(np.float32)
    base = im.mean(1, keepdims=True) if C == 1 else im
    pred = np.clip(base + 0.05 * rng.standard_normal((B, C, H, W)), 0, 1).astype(np.float32)
    conf = (0.05 + 0.95 * rng.random((B, 1, H, W))).astype(np.float32)
    grad = rng.standard_normal((B, C, H, W)).astype(np.float32)
    return [torch.from_numpy(a).cuda() for a in (im, pred, conf, grad)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import inverserenderingofindoorscene_amd as sgr
    if not torch.cuda.is_available():
        raise SystemExit("bilateral_bench needs a GPU")
    configs = [(0, 3, 480, 640, 1)] if args.profile else [(mode, 3 if mode == 0 else 1, H, W, B) for mode in (0, 2, 4) for (H, W) in ((240, 320), (480, 640)) for B in (1, 4)]
    reps, warm = (5, 2) if args.profile else (max(50, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "ms": {}}
    for mode, C, H, W, B in configs:
        P = sgr.BILATERAL_MODES[mode]
        im, pred, conf, grad = inputs(B, C, H, W)
        pred.requires_grad_(True)
        conf.requires_grad_(True)

        def fwd():
            with torch.no_grad():
                return sgr.bilateral_solve(im, pred, conf, **P["grid"], **P["bs"])

        def fwdbwd():
            out = sgr.bilateral_solve(im, pred, conf, **P["grid"], **P["bs"])
            return torch.autograd.grad(out, [pred, conf], grad_outputs=grad)

        nv = torch.ops.sgrender.bilateral_grid(im, *[float(P["grid"][k]) for k in ("sigma_luma", "sigma_chroma", "sigma_spatial")])[4].cpu().tolist()
        for name, f in (("fwd", fwd), ("fwd_bwd", fwdbwd)):
            for _ in range(warm):
                f()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for e0, e1 in ev:
                e0.record()
                f()
                e1.record()
            torch.cuda.synchronize()
            t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
            q = statistics.quantiles(t, n=10)
            key = f"mode{mode}_C{C}_{H}x{W}_B{B}_{name}"
            rec["ms"][key] = dict(median=statistics.median(t), p10=q[0], p90=q[-1], nvertices=nv)
            print(f"{key:34s} median {statistics.median(t):8.3f} ms  p10 {q[0]:8.3f}  p90 {q[-1]:8.3f}  vertices/image {nv}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
