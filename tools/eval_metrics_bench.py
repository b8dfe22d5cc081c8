"""Times of the evaluation-metric operators (sgr.whdr, sgr.normal_angle_error, sgr.depth_log_rmse) at the fine-tuning sizes, batch 16:
one IIW-sized albedo (341 x 512 bytes) with 800 + 800 judgements per image; NYU normals and NYU depth from 240 x 320 to 480 x 640.

    python tools/eval_metrics_bench.py [--reps 80] [--warmup 5] [--out FILE.txt]
    python tools/eval_metrics_bench.py --step whdr          # one step in this process
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/eval_metrics_bench.py --step kernels      # the kernel split, a run of its own

Without --step the tool never touches the GPU itself: every step runs in a fresh child process under a time limit of its own, one after the
other, and the first step that fails, faults or runs out of time ends the run (nothing more is started on the device).

Three candidates per step.  `fused` (the operator) and `eager` (a PyTorch-ROCm composition on the same device tensors: F.interpolate's
bilinear rule, not OpenCV's, and torch.median's lower middle element, not numpy's mean of two -- the same work, not the same bits) alternate
in one process, device events around each call, the median of >= 80 with the min-max spread.  `host` is the reference's route: `.cpu()` of
the predictions plus the checker's fp32 numpy (tests/eval_metrics_checker.py), wall clock, best of 3: a column of its own, not comparable
event for event."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B = 16
STEPS = (("whdr", 240), ("normal", 300), ("depth", 240))      # (step, its time limit in seconds)


def timed(fns, reps, warm):
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
            t[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: sorted(v) for k, v in t.items()}


def wall(f, n=3):
    best = float("inf")
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        best = min(best, time.perf_counter() - t0)
    return best * 1e6


def report(step, t, host_us):
    s = {k: (statistics.median(v), v[0], v[-1]) for k, v in t.items()}
    for k, (med, lo, hi) in s.items():
        print(f"{step:7s} {k:6s} median {med:10.1f} us   min {lo:10.1f}   max {hi:10.1f}   (n = {len(t[k])})")
    overlap = s["fused"][2] >= s["eager"][1]
    print(f"{step:7s} fused / eager = {s['fused'][0] / s['eager'][0]:.3f}{'   SPREADS OVERLAP' if overlap else ''}{'   FUSED IS SLOWER' if s['fused'][0] > s['eager'][0] else ''}")
    print(f"{step:7s} host   best of 3 {host_us:10.1f} us wall clock (.cpu() + the checker's fp32 numpy)")


def step_whdr(args):
    import torch
    import eval_metrics_checker as K
    import inverserenderingofindoorscene_amd as sgr
    im, point, weight, label, num = K.draw_whdr(B, 341, 512, 1600, 1, nums=[1600] * B, garbage=False)
    d = [torch.from_numpy(v).cuda() for v in (im, point, weight, label, num)]
    bi = torch.arange(B, device="cuda")[:, None]

    def eager():
        lum = (d[0].float() / 255.0).mean(dim=3).clamp_min(1e-10)
        p = d[1].long()
        l1, l2 = lum[bi, p[..., 0], p[..., 1]], lum[bi, p[..., 2], p[..., 3]]
        alg = torch.where(l2 / l1 > 1.1, 1, torch.where(l1 / l2 > 1.1, 2, 0))
        w = d[2].double()
        wrong, eq = (alg != d[3]).double() * w, (d[3] == 0).double()
        return (wrong.sum(1) / w.sum(1), (wrong * eq).sum(1) / ((w * eq).sum(1) + 1e-10), (wrong * (1 - eq)).sum(1) / ((w * (1 - eq)).sum(1) + 1e-10))
    t = timed(dict(fused=lambda: sgr.whdr(*d), eager=eager), args.reps, args.warmup)
    report("whdr", t, wall(lambda: K.whdr(K.reflectance_of(d[0].cpu().numpy(), np.float32), point, weight, label, num, dtype=np.float32), 1))


def step_normal(args):
    import torch
    import torch.nn.functional as F
    import eval_metrics_checker as K
    import inverserenderingofindoorscene_amd as sgr
    pred, gt, mask = (torch.from_numpy(v).cuda() for v in K.draw_normal(B, 240, 320, 480, 640, 2))

    def eager():
        p = F.interpolate(pred, size=(480, 640), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        g = (gt.float() - 127.5) / 127.5
        g = g / g.norm(dim=3, keepdim=True)
        theta = torch.acos((p * g).sum(3).clamp(-1, 1)) / torch.pi * 180
        m = mask.amin(dim=3) == 255
        mean = (theta.double() * m).sum((1, 2)) / m.sum((1, 2))
        med = torch.where(m, theta, torch.inf).flatten(1).sort(dim=1).values.gather(1, ((m.sum((1, 2)) - 1) // 2)[:, None])
        return mean, med
    t = timed(dict(fused=lambda: sgr.normal_angle_error(pred, gt, mask), eager=eager), args.reps, args.warmup)
    report("normal", t, wall(lambda: K.normal_angle(pred.cpu().numpy(), gt.cpu().numpy(), mask.cpu().numpy(), np.float32)))


def step_depth(args):
    import torch
    import torch.nn.functional as F
    import eval_metrics_checker as K
    import inverserenderingofindoorscene_amd as sgr
    pred, gt = (torch.from_numpy(v).cuda() for v in K.draw_depth(B, 240, 320, 480, 640, 3))

    def eager():
        m = ((gt > 1) & (gt < 10)).float()
        d = torch.log(F.interpolate(pred[:, None], size=(480, 640), mode="bilinear", align_corners=False)[:, 0] + 1e-20)
        g = torch.log(gt + 1e-20)
        d, g = d - d.mean((1, 2), keepdim=True), g - g.mean((1, 2), keepdim=True)
        return torch.sqrt(((d - g) ** 2 * m).sum((1, 2)) / m.sum((1, 2)))
    t = timed(dict(fused=lambda: sgr.depth_log_rmse(pred, gt), eager=eager), args.reps, args.warmup)
    report("depth", t, wall(lambda: K.depth_log_rmse(pred.cpu().numpy(), gt.cpu().numpy(), np.float32)))


def step_kernels(args):
    """the three operators alone, 20 calls each: the process a `rocprofv3 --kernel-trace --stats` run of its own wraps for the kernel split"""
    import torch
    import eval_metrics_checker as K
    import inverserenderingofindoorscene_amd as sgr
    w = [torch.from_numpy(v).cuda() for v in K.draw_whdr(B, 341, 512, 1600, 1, nums=[1600] * B, garbage=False)]
    n = [torch.from_numpy(v).cuda() for v in K.draw_normal(B, 240, 320, 480, 640, 2)]
    d = [torch.from_numpy(v).cuda() for v in K.draw_depth(B, 240, 320, 480, 640, 3)]
    for _ in range(20):
        sgr.whdr(*w)
        sgr.normal_angle_error(*n)
        sgr.depth_log_rmse(*d)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", default="", choices=("", "kernels") + tuple(s for s, _ in STEPS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.step:
        dict(whdr=step_whdr, normal=step_normal, depth=step_depth, kernels=step_kernels)[args.step](args)
        return 0
    lines = []
    for step, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--warmup", str(args.warmup)],
                           capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        lines.append(r.stdout)
        if r.returncode != 0:      # a failure, a fault or the time limit: nothing more is started on the device
            sys.stderr.write(r.stderr[-3000:])
            print(f"step {step} ended with status {r.returncode}: stopping")
            return r.returncode
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
