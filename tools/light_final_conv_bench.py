"""Times of the light decoders' final pad + 3x3 convolution (sgr.light_final_conv) against the eager PyTorch composition of the same line of the
reference (models.py:334) on the same GPU, at 16 x 128 x 120x160 with 36 and with 12 outputs, forward and forward + backward.  Candidates:

    ours      sgr.light_final_conv
    eager     F.conv2d(F.pad(y, (1, 1, 1, 1), mode='replicate'), Wt, bias)
    eager2x   forward only: the eager form as the reference writes it, the convolution called twice (models.py:334 and :336)

    python tools/light_final_conv_bench.py [--reps 80] [--warmup 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/light_final_conv_bench.py --profile     # ours only, few repetitions

Method: device events around each call, warm-up, median of >= 80, the candidates alternating in one process; the min-max spread of the
repetitions is printed beside each median.  The floors come from the shapes at the measured fp32 matrix peak of 155 TFLOP/s with the outputs
padded to a multiple of 16: forward 2 B H W 9 C Opad, data gradient 2 B H W 9 C O, weight gradient as the forward.
The eager backward uses the pad's atomic scatter, which PyTorch lists as non-deterministic; ours is a gather."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 155.0
SHAPES = [(16, 128, 36, 120, 160), (16, 128, 12, 120, 160)]


def floors_us(B, C, O, H, W):
    """-> (forward, forward + backward) compute floors in microseconds"""
    opad = (O + 15) // 16 * 16
    fwd, data, wgt = (2.0 * B * H * W * 9 * C * n for n in (opad, O, opad))
    us = lambda flop: flop / (PEAK_TFLOPS * 1e12) * 1e6
    return us(fwd), us(fwd + data + wgt)


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
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import inverserenderingofindoorscene_amd as sgr
    if not torch.cuda.is_available():
        raise SystemExit("light_final_conv_bench needs a GPU")
    reps, warm = (5, 2) if args.profile else (max(80, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "ms": {}, "floor_us": {}}
    for B, C, O, H, W in SHAPES:
        name = f"{B}x{C}x{H}x{W}_O{O}"
        g = torch.Generator().manual_seed(B + O)
        y = torch.randn(B, C, H, W, generator=g).cuda().requires_grad_(True)
        Wt = (torch.randn(O, C, 3, 3, generator=g) / (9.0 * C) ** 0.5).cuda().requires_grad_(True)
        bias = (0.1 * torch.randn(O, generator=g)).cuda().requires_grad_(True)
        ct = torch.randn(B, O, H, W, generator=g).cuda()
        leaves = [y, Wt, bias]
        eager = lambda: F.conv2d(F.pad(y, (1, 1, 1, 1), mode="replicate"), Wt, bias)
        cands = dict(ours=lambda: sgr.light_final_conv(y, Wt, bias))
        if not args.profile:
            cands["eager"] = eager

        def fwd(f):
            def run():
                with torch.no_grad():
                    return f()
            return run

        def fwdbwd(f):
            return lambda: torch.autograd.grad(f(), leaves, grad_outputs=ct)
        fns = {}
        for k, f in cands.items():
            fns[f"{k}_fwd"], fns[f"{k}_fwd_bwd"] = fwd(f), fwdbwd(f)
        if not args.profile:
            def twice():
                with torch.no_grad():
                    p = F.pad(y, (1, 1, 1, 1), mode="replicate")
                    q = F.pad(y, (1, 1, 1, 1), mode="replicate")
                    return F.conv2d(p, Wt, bias), F.conv2d(q, Wt, bias)
            fns["eager2x_fwd"] = twice
        t = timed(fns, reps, warm)
        fl = floors_us(B, C, O, H, W)
        rec["floor_us"][name] = dict(forward=fl[0], forward_backward=fl[1])
        for k, v in t.items():
            med = statistics.median(v)
            rec["ms"][f"{name}_{k}"] = dict(median=med, min=v[0], max=v[-1])
            cand, what = k.split("_", 1)
            note = ""
            if cand == "ours":
                floor = fl[0] if what == "fwd" else fl[1]
                note = f"compute floor {floor:.0f} us at {PEAK_TFLOPS:.0f} TFLOP/s (share {floor / (med * 1e3):.2f})"
            print(f"{name + ' ' + k:40s} median {med * 1e3:9.1f} us  min {v[0] * 1e3:9.1f}  max {v[-1] * 1e3:9.1f}  {note}")
        if not args.profile:
            for what, other in (("fwd", "eager"), ("fwd_bwd", "eager"), ("fwd", "eager2x")):
                ours, ea = rec["ms"][f"{name}_ours_{what}"], rec["ms"][f"{name}_{other}_{what}"]
                s = ea["median"] / ours["median"]
                rec["ms"][f"{name}_speedup_{what}_vs_{other}"] = s
                if s >= 1:
                    verdict = "the difference exceeds the spread" if ea["min"] > ours["max"] else "THE SPREADS OVERLAP"
                else:
                    verdict = "SLOWER THAN EAGER" + ("" if ours["min"] > ea["max"] else ", the spreads overlap")
                print(f"{name + ' ' + what + ' vs ' + other:40s} {other} / ours = {s:.2f}x  ({verdict})")
        del y, Wt, bias, ct, leaves
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
