"""Times of sgr.pil_resize at the loaders' sizes: batch 16 of 480 x 640 x 3 to 240 x 320 (dataLoader.py:223-224) and one 341 x 512 IIW
photograph to its 240 x 320 crop of 240 x 361 (iiwDataLoader.py:112-134).

    python tools/pil_resize_bench.py [--reps 80] [--warmup 5] [--out FILE.txt]
    python tools/pil_resize_bench.py --step loader          # one step in this process

Without --step the tool never touches the GPU itself: every step runs in a fresh child process under a time limit of its own, one after the
other, and the first step that fails, faults or runs out of time ends the run (nothing more is started on the device).

`tiled` and `two_pass` alternate in one process, device events around each call, the median of >= 80 with the min-max spread.  In columns of
their own, not comparable event for event: `host`, the thing replaced -- ``Image.resize`` on 16 threads, wall clock, best of 3, where Pillow
imports (the machine is named) --, and `upload`, the pinned host-to-device copy of the full-size against the resized uint8 batch: what moving
the resize to the device adds to the copy."""
import argparse
import os
import platform
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 16
STEPS = (("loader", 240), ("iiw", 240))      # (step, its time limit in seconds)


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


def report(step, t):
    s = {k: (statistics.median(v), v[0], v[-1]) for k, v in t.items()}
    for k, (med, lo, hi) in s.items():
        print(f"{step:7s} {k:14s} median {med:10.1f} us   min {lo:10.1f}   max {hi:10.1f}   (n = {len(t[k])})")
    return s


def compare(step, s, a, b):
    overlap = s[a][2] >= s[b][1] and s[b][2] >= s[a][1]
    print(f"{step:7s} {a} / {b} = {s[a][0] / s[b][0]:.3f}{'   SPREADS OVERLAP' if overlap else ''}")


def host_resize(step, images, size, crop=None):
    try:
        from PIL import Image
    except ImportError:
        print(f"{step:7s} host           Pillow does not import on {platform.node() or 'this machine'}: not timed here")
        return
    pims = [Image.fromarray(a, "RGB") for a in images]

    def one(p):
        out = np.asarray(p.resize(size, Image.Resampling.LANCZOS))
        return out if crop is None else out[crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
    with ThreadPoolExecutor(16) as pool:
        us = wall(lambda: list(pool.map(one, pims)))
    print(f"{step:7s} host           best of 3 {us:10.1f} us wall clock (Image.resize of {len(pims)} image(s) on 16 threads, Pillow {Image.__version__}, "
          f"{platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible)")


def upload(step, full, small, reps, warm):
    import torch
    pf, ps = torch.from_numpy(full).pin_memory(), torch.from_numpy(small).pin_memory()
    df, ds = torch.empty_like(pf, device="cuda"), torch.empty_like(ps, device="cuda")
    s = report(step, timed({"upload full": lambda: df.copy_(pf, non_blocking=True), "upload resized": lambda: ds.copy_(ps, non_blocking=True)}, reps, warm))
    print(f"{step:7s} upload full - upload resized = {s['upload full'][0] - s['upload resized'][0]:.1f} us ({full.nbytes} against {small.nbytes} bytes)")


def step_loader(args):
    import torch
    import inverserenderingofindoorscene_amd as sgr
    rng = np.random.default_rng(1)
    im = rng.integers(0, 256, (B, 480, 640, 3), dtype=np.uint8)
    d = torch.from_numpy(im).cuda()
    assert torch.equal(sgr.pil_resize(d, (320, 240), path="tiled"), sgr.pil_resize(d, (320, 240), path="two_pass"))
    s = report("loader", timed({p: (lambda p=p: sgr.pil_resize(d, (320, 240), path=p)) for p in ("tiled", "two_pass")}, args.reps, args.warmup))
    compare("loader", s, "tiled", "two_pass")
    small = sgr.pil_resize(d, (320, 240)).cpu().numpy()
    upload("loader", im, small, args.reps, args.warmup)
    host_resize("loader", list(im), (320, 240))


def step_iiw(args):
    import torch
    import inverserenderingofindoorscene_amd as sgr
    rng = np.random.default_rng(2)
    im = rng.integers(0, 256, (341, 512, 3), dtype=np.uint8)
    d = torch.from_numpy(im).cuda()
    win = (0, 20, 240, 320)
    assert torch.equal(sgr.pil_resize(d, (361, 240), window=win, path="tiled"), sgr.pil_resize(d, (361, 240), window=win, path="two_pass"))
    fns = {p: (lambda p=p: sgr.pil_resize(d, (361, 240), window=win, path=p)) for p in ("tiled", "two_pass")}
    fns["two_pass whole"] = lambda: sgr.pil_resize(d, (361, 240), path="two_pass")[:, 20:340]
    s = report("iiw", timed(fns, args.reps, args.warmup))
    compare("iiw", s, "tiled", "two_pass")
    small = sgr.pil_resize(d, (361, 240), window=win).cpu().numpy()
    upload("iiw", im, small, args.reps, args.warmup)
    host_resize("iiw", [im], (361, 240), win)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        {"loader": step_loader, "iiw": step_iiw}[args.step](args)
        return 0
    lines = []
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"step {step} ended with status {r.returncode}: nothing more is started")
            return r.returncode
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
