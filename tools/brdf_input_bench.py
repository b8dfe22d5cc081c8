"""Times of the cascade-1 BRDF encoder input (sgr.brdf_encoder_input) against an eager PyTorch composition of the reference's lines
(wrapperBRDF.py:56-100) on the same GPU: batch 16 at 240x320 (BRDF maps 240x320, env grid 120x160: the identity branch) and at 480x640
(BRDF maps 240x320, env grid 120x160: every map resized).

    python tools/brdf_input_bench.py [--reps 80] [--warmup 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/brdf_input_bench.py --profile     # the fused call only, few repetitions

Method: device events around each call, warm-up, median of >= 80, the fused call and the eager form alternating in one process.  The
algorithmic bytes come from the shapes: 4 bn (17 H W written + 3 H W + 8 h w + 6 R C read once).  The fused call's split re-reads on top
of that (reported separately; they may come from the 256 MB Infinity Cache): pass A and pass B each form the pooled image from `im` and
read diffuse / specular before pass C reads them (2 x 3 H W + 2 x 6 R C), and pass A has summed albedo and depth before pass C reads them
(4 h w)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 8.0


def inputs(bn, H, W, h, w, R, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    normal = torch.randn(bn, 3, h, w, generator=g)
    x = (1.1 * u(bn, 3, H, W), u(bn, 3, h, w), normal / normal.norm(dim=1, keepdim=True), u(bn, 1, h, w), 0.5 + 4 * u(bn, 1, h, w), 0.8 * u(bn, 3, R, C),
         0.3 * u(bn, 3, R, C))
    return [t.cuda() for t in x]


def eager_diffspec(diff, spec, im):
    """models.py:23-84 restated in eager PyTorch"""
    nb, n = diff.shape[0], diff[0].numel()
    mask = (im < 0.9).float()
    d, s, i = (diff * mask).reshape(nb, -1), (spec * mask).reshape(nb, -1), (im * mask).reshape(nb, -1)
    a11, a22, a12 = (d * d).sum(1), (s * s).sum(1), (d * s).sum(1)
    frac = a11 * a22 - a12 * a12
    b1, b2 = (d * i).sum(1), (s * i).sum(1)
    c1 = (b1 * a22 - b2 * a12) / torch.clamp(frac, min=1e-2)
    c2 = (-b1 * a12 + a11 * b2) / torch.clamp(frac, min=1e-2)
    c3 = torch.clamp(b1 / torch.clamp(a11, min=1e-5), 0.001, 1000)
    ind = ((frac / n) > 1e-2).float()
    cd = torch.clamp(ind * c1 + (1 - ind) * c3, 0, 1000).reshape(nb, 1, 1, 1)
    cs = torch.clamp(ind * c2, 0, 1000).reshape(nb, 1, 1, 1)
    ds, ss = cd * diff, cs * spec
    r = torch.clamp(ds + ss, 0, 1).reshape(nb, -1)
    cim = torch.clamp((r * im.reshape(nb, -1)).sum(1) / torch.clamp((r * r).sum(1), min=1e-5), 0.001, 1000).reshape(nb, 1, 1, 1)
    return cim * ds, cim * ss


def eager_input(im, albedo, normal, rough, depth, diffuse, spec):
    """wrapperBRDF.py:56-100 restated in eager PyTorch"""
    H, W = im.shape[2], im.shape[3]
    up = lambda t: F.interpolate(t, [H, W], mode="bilinear") if t.shape[2] < H or t.shape[3] < W else t
    albedo, normal, rough, depth = up(albedo), up(normal), up(rough), up(depth)
    small = F.adaptive_avg_pool2d(im, (diffuse.shape[2], diffuse.shape[3]))
    diffuse, spec = eager_diffspec(diffuse, spec, small)
    diffuse, spec = up(diffuse), up(spec)
    bn = im.shape[0]
    norm = lambda t: (t.reshape(bn, -1) / torch.clamp(t.reshape(bn, -1).mean(1), min=1e-10).unsqueeze(1) / 3.0).reshape(t.shape)
    return torch.cat([im, norm(albedo), normal, rough, norm(depth), diffuse, spec], 1)


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
        raise SystemExit("brdf_input_bench needs a GPU")
    reps, warm = (5, 2) if args.profile else (max(80, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "ms": {}, "bytes": {}}
    for bn, H, W, h, w, R, C in ((16, 240, 320, 240, 320, 120, 160), (16, 480, 640, 240, 320, 120, 160)):
        x = inputs(bn, H, W, h, w, R, C)
        written, read_once = 4 * bn * 17 * H * W, 4 * bn * (3 * H * W + 8 * h * w + 6 * R * C)
        reread = 4 * bn * (2 * 3 * H * W + 4 * h * w + 2 * 6 * R * C)
        floor_us = (written + read_once) / (HBM_TBPS * 1e12) * 1e6
        tag = f"input_B{bn}_{H}x{W}_maps{h}x{w}_env{R}x{C}"
        rec["bytes"][tag] = dict(written=written, read_once=read_once, reread_by_the_split=reread, floor_us_at_8TBps=floor_us)
        with torch.no_grad():
            got, want = sgr.brdf_encoder_input(*x)[0], eager_input(*x)
            rec["bytes"][tag]["rel_l2_fused_vs_eager"] = float((got.double() - want.double()).norm() / want.double().norm())
            del got, want
        fns = dict(fused=lambda: sgr.brdf_encoder_input(*x))
        if not args.profile:
            def eager():
                with torch.no_grad():
                    return eager_input(*x)
            fns["eager"] = eager
        t = timed(fns, reps, warm)
        for k, v in t.items():
            q = statistics.quantiles(v, n=10)
            med = statistics.median(v)
            rec["ms"][f"{tag}_{k}"] = dict(median=med, p10=q[0], p90=q[-1])
            note = ""
            if k == "fused":
                note = (f"algorithmic {(written + read_once) / 1e6:.1f} MB (+ {reread / 1e6:.1f} MB re-read by the split): floor {floor_us:.1f} us at {HBM_TBPS} TB/s, "
                        f"achieved share {floor_us / (med * 1e3):.2f}; rel-L2 against the eager form {rec['bytes'][tag]['rel_l2_fused_vs_eager']:.1e}")
                rec["bytes"][tag]["achieved_share_of_floor"] = floor_us / (med * 1e3)
            print(f"{tag + '_' + k:52s} median {med * 1e3:9.1f} us  p10 {q[0] * 1e3:9.1f}  p90 {q[-1] * 1e3:9.1f}  {note}")
        if not args.profile:
            s = rec["ms"][tag + "_eager"]["median"] / rec["ms"][tag + "_fused"]["median"]
            rec["ms"][tag + "_speedup"] = s
            print(f"{tag:52s} eager / fused = {s:.1f}x")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
