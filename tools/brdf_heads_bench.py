"""Times of the BRDF decoder output heads (sgr.brdf_heads) against an eager PyTorch restatement of the reference's lines
(models.py:189-203 for the four decoders, plus the wrappers' 0.5 (x + 1) on albedo and depth) on the same GPU: batch 16 at 240x320 (the
trainBRDF.py defaults) and at 480x640, forward and forward + backward.

    python tools/brdf_heads_bench.py [--reps 80] [--warmup 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/brdf_heads_bench.py --profile     # the fused calls only, few repetitions

Method: device events around each call, warm-up, median of >= 80, the fused call and the eager form alternating in one process; the
min-max spread of the repetitions is printed beside each median.  The algorithmic byte counts come from the shapes, with all four terms:
forward reads 12 planes and writes 8, backward reads the 12 planes and the 8 cotangent planes and writes 12.  Each fused time is shown
with the share of that floor at 8 TB/s (the HBM peak) and at 6.29 TB/s (what this project measured for a float4 copy)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 8.0
COPY_TBPS = 6.29


def inputs(B, H, W, seed=0):
    """pre-activations 2 N(0,1) (depth: 2 sqrt(3) N(0,1): its channel mean is 2 N(0,1)), about 18 % saturated; N(0,1) cotangents"""
    g = torch.Generator().manual_seed(seed)
    xs = [(2.0 * 3 ** 0.5 if k == 3 else 2.0) * torch.randn(B, 3, H, W, generator=g) for k in range(4)]
    cts = [torch.randn(B, c, H, W, generator=g) for c in (3, 3, 1, 1)]
    return [x.cuda() for x in xs], [c.cuda() for c in cts]


def eager_heads(xa, xn, xr, xd):
    """models.py:189-203 for modes 0, 1, 2, 4 and the wrappers' 0.5 * (x + 1), restated in eager PyTorch"""
    albedo = 0.5 * (torch.clamp(1.01 * torch.tanh(xa), -1, 1) + 1)
    t = torch.clamp(1.01 * torch.tanh(xn), -1, 1)
    norm = torch.sqrt(torch.sum(t * t, dim=1).unsqueeze(1)).expand_as(t)
    normal = t / torch.clamp(norm, min=1e-6)
    rough = torch.mean(torch.clamp(1.01 * torch.tanh(xr), -1, 1), dim=1).unsqueeze(1)
    depth = 0.5 * (torch.clamp(1.01 * torch.tanh(torch.mean(xd, dim=1).unsqueeze(1)), -1, 1) + 1)
    return albedo, normal, rough, depth


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


def report(rec, key, t, note=""):
    rec["ms"][key] = dict(median=statistics.median(t), min=t[0], max=t[-1])
    print(f"{key:40s} median {statistics.median(t) * 1e3:9.1f} us  min {t[0] * 1e3:9.1f}  max {t[-1] * 1e3:9.1f}  {note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import inverserenderingofindoorscene_amd as sgr
    if not torch.cuda.is_available():
        raise SystemExit("brdf_heads_bench needs a GPU")
    reps, warm = (5, 2) if args.profile else (max(80, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "ms": {}, "bytes": {}}
    for B, H, W in ((16, 240, 320), (16, 480, 640)):
        xs, cts = inputs(B, H, W)
        live = [x.clone().requires_grad_(True) for x in xs]
        plane = B * H * W * 4
        b_fwd, b_bwd = (12 + 8) * plane, (12 + 8 + 12) * plane
        rec["bytes"][f"{B}x{H}x{W}"] = dict(forward=b_fwd, backward=b_bwd)

        def fused_fwd():
            with torch.no_grad():
                return sgr.brdf_heads(*xs)

        def fused_fwdbwd():
            return torch.autograd.grad(sgr.brdf_heads(*live), live, grad_outputs=cts)

        def eager_fwd():
            with torch.no_grad():
                return eager_heads(*xs)

        def eager_fwdbwd():
            return torch.autograd.grad(eager_heads(*live), live, grad_outputs=cts)

        fns = dict(fused_fwd=fused_fwd, fused_fwd_bwd=fused_fwdbwd)
        if not args.profile:
            fns.update(eager_fwd=eager_fwd, eager_fwd_bwd=eager_fwdbwd)
        t = timed(fns, reps, warm)
        tag = f"heads_B{B}_{H}x{W}_"
        for k, v in t.items():
            note = ""
            if k.startswith("fused"):
                nbytes = b_fwd if k == "fused_fwd" else b_fwd + b_bwd
                med = statistics.median(v) * 1e3
                f8, f6 = nbytes / (HBM_TBPS * 1e12) * 1e6, nbytes / (COPY_TBPS * 1e12) * 1e6
                note = f"algorithmic {nbytes / 1e6:.1f} MB: floor {f8:.1f} us at {HBM_TBPS} TB/s (share {f8 / med:.2f}), {f6:.1f} us at {COPY_TBPS} TB/s (share {f6 / med:.2f})"
            report(rec, tag + k, v, note)
        if not args.profile:
            for k in ("fwd", "fwd_bwd"):
                fu, ea = rec["ms"][tag + "fused_" + k], rec["ms"][tag + "eager_" + k]
                s = ea["median"] / fu["median"]
                rec["ms"][tag + "speedup_" + k] = s
                clear = ea["min"] > fu["max"]
                print(f"{tag + k:40s} eager / fused = {s:.1f}x   slowest fused {fu['max'] * 1e3:.1f} us {'<' if clear else '>='} fastest eager {ea['min'] * 1e3:.1f} us"
                      f"  ({'the difference exceeds the spread' if clear else 'THE SPREADS OVERLAP'})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
