"""Times of the encoders' pad + 4x4 stride-2 convolution (sgr.encoder_conv) against the eager PyTorch composition of the same lines of the
reference (models.py:122-123, 254, 262) on the same GPU, at batch 16 and the reference's training size: the five layers the operator covers,
two of them with a cascade-0 and a cascade-1 input width, forward and forward + backward.  Candidates:

    ours      sgr.encoder_conv(x, Wt, bias, padding)
    eager     F.conv2d(F.pad(x, (1, 1, 1, 1), mode=padding), Wt, bias, stride=2)

    python tools/encoder_conv_bench.py [--reps 80] [--warmup 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/encoder_conv_bench.py --profile     # ours only, few repetitions
    python tools/encoder_conv_bench.py --sources [--profile]     # the several-source leg alone (below)

``--sources``: encoderLight.conv1 at cascade 1 as the reference feeds it -- the 64 ``preProcess`` channels and the 7 SGNum channels of
``envmapsPreBatch`` as two tensors (models.py:254-262) -- at batch 16, 120x160, 128 outputs, replicate, splits (64, 84) and (64, 7):

    cat_ours      sgr.encoder_conv_cat([x1, x2], Wt, bias)                        no concatenated copy
    cat_then_ours sgr.encoder_conv(torch.cat([x1, x2], 1), Wt, bias)              what the single-source operator offers
    eager         F.conv2d(F.pad(torch.cat([x1, x2], 1), ...), Wt, bias, stride=2)

forward, and forward + backward with only the first source requiring grad (``first``: what trainLight.py at cascade 1 does -- the envmaps
are data) and with both (``both``).  The floor is the single-source floor of the summed channels, with the data gradient's share scaled to
the channels that want one.

Method: device events around each call, warm-up, median of >= 80, the candidates alternating in one process; the min-max spread of the
repetitions is printed beside each median.  encoder0.conv1 is measured without the data gradient, as in training (its input is the image).
The floors come from the shapes: 2 B Ho Wo O 16 C FLOP for the forward and as much again for each gradient at the
measured fp32 matrix peak of 155 TFLOP/s, or the compulsory traffic (x and out once for the forward; the cotangent and x again for the
weight gradient, the cotangent and dx for the data gradient) at 8 TB/s where that is more.  The eager backward of the replicate pad is an
atomic scatter, which PyTorch lists as non-deterministic; ours is a gather."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS, PEAK_TBS = 155.0, 8.0
B = 16
# (layer, padding, C, O, H, W of the input, whether the data gradient is wanted)
SHAPES = [("encoder0.conv1_c0", "replicate", 3, 64, 240, 320, False), ("encoder0.conv1_c1", "replicate", 17, 64, 240, 320, False),
          ("encoder0.conv2", "zeros", 64, 128, 120, 160, True), ("encoderLight.pre1", "replicate", 11, 32, 480, 640, True),
          ("encoderLight.pre5", "zeros", 32, 64, 240, 320, True), ("encoderLight.conv1_c0", "replicate", 64, 128, 120, 160, True),
          ("encoderLight.conv1_c1", "replicate", 148, 128, 120, 160, True)]


def floors_us(C, O, H, W, need_dx):
    """-> (forward, forward + backward) floors in microseconds: the larger of the compute and the traffic floor"""
    Ho, Wo = H // 2, W // 2
    flop = 2.0 * B * Ho * Wo * O * 16 * C
    x, out = 4.0 * B * C * H * W, 4.0 * B * O * Ho * Wo
    us = lambda fl, by: max(fl / (PEAK_TFLOPS * 1e12), by / (PEAK_TBS * 1e12)) * 1e6
    fwd = us(flop, x + out)
    bwd = us(flop, x + out) + us(0.0, out) + (us(flop, x + out) if need_dx else 0.0)      # dWt, dbias, dx
    return fwd, fwd + bwd


def sources_leg(sgr, args, rec):
    """the --sources leg: three candidates alternating, forward / forward + backward (first source's dx only, both)"""
    reps, warm = (5, 2) if args.profile else (max(80, args.reps), args.warmup)
    O, H, W = 128, 120, 160
    for split in ((64, 84), (64, 7)):
        C = sum(split)
        name = f"encoderLight.conv1_c1_{split[0]}+{split[1]}to{O}_{H}x{W}"
        g = torch.Generator().manual_seed(C + O)
        x1, x2 = (torch.randn(B, c, H, W, generator=g).cuda() for c in split)
        Wt = (torch.randn(O, C, 4, 4, generator=g) / (16.0 * C) ** 0.5).cuda().requires_grad_(True)
        bias = (0.1 * torch.randn(O, generator=g)).cuda().requires_grad_(True)
        ct = torch.randn(B, O, H // 2, W // 2, generator=g).cuda()
        cands = dict(cat_ours=lambda a, b: sgr.encoder_conv_cat([a, b], Wt, bias))
        if not args.profile:
            cands["cat_then_ours"] = lambda a, b: sgr.encoder_conv(torch.cat([a, b], 1), Wt, bias)
            cands["eager"] = lambda a, b: F.conv2d(F.pad(torch.cat([a, b], 1), (1, 1, 1, 1), mode="replicate"), Wt, bias, stride=2)
        a1, b1 = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)

        def fwd(f):
            def run():
                with torch.no_grad():
                    return f(x1, x2)
            return run
        fns = {}
        for k, f in cands.items():
            fns[f"{k}|fwd"] = fwd(f)
            fns[f"{k}|fwd_bwd_first"] = lambda f=f: torch.autograd.grad(f(a1, x2), [a1, Wt, bias], grad_outputs=ct)
            fns[f"{k}|fwd_bwd_both"] = lambda f=f: torch.autograd.grad(f(a1, b1), [a1, b1, Wt, bias], grad_outputs=ct)
        t = timed(fns, reps, warm)
        f_fwd, f_all = floors_us(C, O, H, W, True)
        dx_share = floors_us(C, O, H, W, True)[1] - floors_us(C, O, H, W, False)[1]
        floor = dict(fwd=f_fwd, fwd_bwd_first=f_all - dx_share * (1.0 - split[0] / C), fwd_bwd_both=f_all)
        rec["floor_us"][name] = floor
        for k, v in t.items():
            med = statistics.median(v)
            cand, what = k.split("|")
            rec["ms"][f"{name}_{cand}_{what}"] = dict(median=med, min=v[0], max=v[-1])
            note = f"floor {floor[what]:.0f} us (share {floor[what] / (med * 1e3):.2f})" if cand == "cat_ours" else ""
            print(f"{name + ' ' + cand + ' ' + what:74s} median {med * 1e3:9.1f} us  min {v[0] * 1e3:9.1f}  max {v[-1] * 1e3:9.1f}  {note}", flush=True)
        for what in floor if not args.profile else ():
            ours = rec["ms"][f"{name}_cat_ours_{what}"]
            for other in ("cat_then_ours", "eager"):
                o = rec["ms"][f"{name}_{other}_{what}"]
                s = o["median"] / ours["median"]
                rec["ms"][f"{name}_speedup_{what}_vs_{other}"] = s
                if s >= 1:
                    verdict = "the difference exceeds the spread" if o["min"] > ours["max"] else "THE SPREADS OVERLAP"
                else:
                    verdict = "THE NEW CALL IS SLOWER" + ("" if ours["min"] > o["max"] else ", the spreads overlap")
                print(f"{name + ' ' + what + ' vs ' + other:74s} {other} / cat_ours = {s:.2f}x  ({verdict})", flush=True)
        del x1, x2, a1, b1, Wt, bias, ct
        torch.cuda.empty_cache()


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
    ap.add_argument("--sources", action="store_true", help="the several-source leg (sgr.encoder_conv_cat) instead of the single-source layers")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import inverserenderingofindoorscene_amd as sgr
    if not torch.cuda.is_available():
        raise SystemExit("encoder_conv_bench needs a GPU")
    reps, warm = (5, 2) if args.profile else (max(80, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "ms": {}, "floor_us": {}}
    if args.sources:
        sources_leg(sgr, args, rec)
    for layer, padding, C, O, H, W, need_dx in () if args.sources else SHAPES:
        name = f"{layer}_{C}to{O}_{H}x{W}"
        g = torch.Generator().manual_seed(C + O)
        x = torch.randn(B, C, H, W, generator=g).cuda().requires_grad_(need_dx)
        Wt = (torch.randn(O, C, 4, 4, generator=g) / (16.0 * C) ** 0.5).cuda().requires_grad_(True)
        bias = (0.1 * torch.randn(O, generator=g)).cuda().requires_grad_(True)
        ct = torch.randn(B, O, H // 2, W // 2, generator=g).cuda()
        leaves = [t for t in (x, Wt, bias) if t.requires_grad]
        mode = "replicate" if padding == "replicate" else "constant"
        cands = dict(ours=lambda: sgr.encoder_conv(x, Wt, bias, padding))
        if not args.profile:
            cands["eager"] = lambda: F.conv2d(F.pad(x, (1, 1, 1, 1), mode=mode), Wt, bias, stride=2)

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
        t = timed(fns, reps, warm)
        fl = floors_us(C, O, H, W, need_dx)
        rec["floor_us"][name] = dict(forward=fl[0], forward_backward=fl[1])
        for k, v in t.items():
            med = statistics.median(v)
            rec["ms"][f"{name}_{k}"] = dict(median=med, min=v[0], max=v[-1])
            cand, what = k.split("_", 1)
            note = ""
            if cand == "ours":
                floor = fl[0] if what == "fwd" else fl[1]
                note = f"floor {floor:.0f} us (share {floor / (med * 1e3):.2f})"
            print(f"{name + ' ' + k:58s} median {med * 1e3:9.1f} us  min {v[0] * 1e3:9.1f}  max {v[-1] * 1e3:9.1f}  {note}", flush=True)
        if not args.profile:
            for what in ("fwd", "fwd_bwd"):
                ours, ea = rec["ms"][f"{name}_ours_{what}"], rec["ms"][f"{name}_eager_{what}"]
                s = ea["median"] / ours["median"]
                rec["ms"][f"{name}_speedup_{what}_vs_eager"] = s
                if s >= 1:
                    verdict = "the difference exceeds the spread" if ea["min"] > ours["max"] else "THE SPREADS OVERLAP"
                else:
                    verdict = "SLOWER THAN EAGER" + ("" if ours["min"] > ea["max"] else ", the spreads overlap")
                print(f"{name + ' ' + what + ' vs eager':58s} eager / ours = {s:.2f}x  ({verdict})", flush=True)
        del x, Wt, bias, ct, leaves
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
