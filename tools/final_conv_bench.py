"""Times of the BRDF decoders' final pad + 3x3 convolution (sgr.final_conv / sgr.group_norm_relu_final_conv) against the eager PyTorch
composition of the same lines of the reference (models.py:183, 187) on the same GPU, at 16 x 64 x 240x320 and 4 x 64 x 480x640, forward and
forward + backward.  Three candidates:

    eager     F.relu(F.group_norm(x)) -> nn.ReplicationPad2d(1) -> F.conv2d
    composed  sgr.group_norm_relu + sgr.final_conv
    fused     sgr.group_norm_relu_final_conv

    python tools/final_conv_bench.py [--reps 80] [--warmup 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/final_conv_bench.py --profile     # composed and fused only, few repetitions

Method: device events around each call, warm-up, median of >= 80, the candidates alternating in one process; the min-max spread of the
repetitions is printed beside each median.  The algorithmic byte counts come from the shapes; each time of ours is
shown with the share of that floor at 8 TB/s (the HBM peak).  The eager backward uses the pad's atomic scatter, which PyTorch lists as
non-deterministic; ours is a gather."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 8.0
SHAPES = [(16, 64, 4, 240, 320), (4, 64, 4, 480, 640)]


def nbytes(B, C, H, W):
    """-> {candidate: (forward, backward)} algorithmic bytes"""
    m, o = B * C * H * W * 4, B * 3 * H * W * 4
    gn_bwd = 5 * m                      # gn_stage_bwd without a skip: pass 1 reads dy, x; pass 2 reads dy, x, writes dx
    conv_bwd = (o + m) + (m + o)        # data: g in, dy out; weights: y (or x) once, g once (its re-reads per input channel stay in cache)
    return dict(fused=(2 * m + o, conv_bwd + gn_bwd), composed=((2 * m + m) + (m + o), conv_bwd + gn_bwd),
                eager=(None, None))


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
        raise SystemExit("final_conv_bench needs a GPU")
    reps, warm = (5, 2) if args.profile else (max(80, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "ms": {}, "bytes": {}}
    pad = torch.nn.ReplicationPad2d(1)
    for B, C, G, H, W in SHAPES:
        name = f"{B}x{C}x{H}x{W}"
        g = torch.Generator().manual_seed(B + H)
        x = torch.randn(B, C, H, W, generator=g).cuda().requires_grad_(True)
        gw = torch.randn(C, generator=g).cuda().requires_grad_(True)
        gb = (0.3 * torch.randn(C, generator=g)).cuda().requires_grad_(True)
        Wt = (torch.randn(3, C, 3, 3, generator=g) / (9.0 * C) ** 0.5).cuda().requires_grad_(True)
        bias = (0.1 * torch.randn(3, generator=g)).cuda().requires_grad_(True)
        ct = torch.randn(B, 3, H, W, generator=g).cuda()
        leaves = [x, gw, gb, Wt, bias]
        cands = dict(fused=lambda: sgr.group_norm_relu_final_conv(x, gw, gb, G, Wt, bias),
                     composed=lambda: sgr.final_conv(sgr.group_norm_relu(x, gw, gb, G), Wt, bias))
        if not args.profile:
            cands["eager"] = lambda: F.conv2d(pad(F.relu(F.group_norm(x, G, gw, gb, 1e-5), True)), Wt, bias)

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
        nb = nbytes(B, C, H, W)
        rec["bytes"][name] = {k: dict(forward=v[0], backward=v[1]) for k, v in nb.items() if v[0]}
        for k, v in t.items():
            med = statistics.median(v)
            rec["ms"][f"{name}_{k}"] = dict(median=med, min=v[0], max=v[-1])
            cand, what = k.split("_", 1)
            note = ""
            if nb[cand][0]:
                n = nb[cand][0] if what == "fwd" else nb[cand][0] + nb[cand][1]
                floor = n / (HBM_TBPS * 1e12) * 1e6
                note = f"algorithmic {n / 1e6:.1f} MB: floor {floor:.1f} us at {HBM_TBPS} TB/s (share {floor / (med * 1e3):.2f})"
            print(f"{name + ' ' + k:40s} median {med * 1e3:9.1f} us  min {v[0] * 1e3:9.1f}  max {v[-1] * 1e3:9.1f}  {note}")
        if not args.profile:
            for cand in ("composed", "fused"):
                for what in ("fwd", "fwd_bwd"):
                    ours, ea = rec["ms"][f"{name}_{cand}_{what}"], rec["ms"][f"{name}_eager_{what}"]
                    s = ea["median"] / ours["median"]
                    rec["ms"][f"{name}_{cand}_speedup_{what}"] = s
                    if s >= 1:
                        verdict = "the difference exceeds the spread" if ea["min"] > ours["max"] else "THE SPREADS OVERLAP"
                    else:
                        verdict = "OURS IS SLOWER" + ("" if ours["min"] > ea["max"] else ", the spreads overlap")
                    print(f"{name + ' ' + cand + ' ' + what:40s} eager / ours = {s:.2f}x  ({verdict})")
        del x, gw, gb, Wt, bias, ct, leaves
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
