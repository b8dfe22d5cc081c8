"""Times of the CNN stage glue (sgr.group_norm_relu / sgr.group_norm_relu_upcat) against the eager PyTorch composition of the same lines of
the reference (models.py:122-127, 160-183) on the same GPU: the six ``encoder0`` norms and the five ``decoder0`` stages of a 240x320 step
at batch 16, forward and forward + backward.

    python tools/gn_stage_bench.py [--reps 80] [--warmup 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/gn_stage_bench.py --profile     # the fused calls only, few repetitions
    python tools/gn_stage_bench.py --dtype bf16 [--out FILE.json]                        # mixed precision, see below
    rocprofv3 --kernel-trace --stats ... -- python tools/gn_stage_bench.py --dtype bf16 --profile
    python tools/gn_stage_bench.py --siblings 4 --only dec_ [--out FILE.json]            # sibling decoders, see below
    python tools/gn_stage_bench.py --siblings 3 --only light_
    rocprofv3 --kernel-trace --stats ... -- python tools/gn_stage_bench.py --siblings 4 --only dec_ --profile

At 240x320 ``decoder0``'s second stage works at 14x20 against a 15x20 skip: the reference's resize branch.  ``dec_dgn2_plain`` times the plain
form there (GroupNorm + ReLU alone, as before the resize was fused); ``dec_dgn2``, ``light_dgn2``, ``light_dgn3`` and ``dec_final`` are the real
stages through sgr.group_norm_relu_resize_upcat / sgr.group_norm_relu_resize against the reference's composition with its ``if`` taken.

Method: device events around each call, warm-up, median of >= 80, the fused call and the eager form alternating in one process; the
min-max spread of the repetitions is printed beside each median.  The algorithmic byte counts come from the shapes:
forward reads x twice (moments, apply) and the skip once and writes the result; backward reads the cotangent and x, writes and re-reads
the masked adjoint (upsampling form only), reads x again (plain form: the cotangent again) and writes dx and dskip.  Each fused time is
shown with the share of that floor at 8 TB/s (the HBM peak).

``--dtype bf16`` takes the same-size stages of the list and alternates three candidates in one process: the bf16
operator; the fp32 operator on the same values; the eager composition under ``torch.autocast('cuda', dtype=torch.bfloat16)`` reading the
same bf16 ``x`` and ``skip`` (autocast runs ``group_norm`` in fp32: it upcasts first).  The algorithmic bytes of the bf16 operator are half
the fp32 stage's, as every tensor it reads and writes is; the masked adjoint that the upsampling backward writes and re-reads stays fp32, so
that form's true floor is a little higher and the printed share understates it.  Every ratio is printed against both other candidates; where the bf16 operator is slower or the spreads overlap the line says
so in capitals.

``--siblings D`` takes the upcat stages of the list (``--only PREFIX`` selects ``dec_`` for ``decoder0``'s four siblings or
``light_`` for ``decoderLight``'s three) and alternates two candidates in one process: ONE call of the sibling form, and ``D`` calls of the
single form on the same tensors, whose backward is one ``torch.autograd.grad`` over the ``D`` results -- autograd then adds the ``D`` maps of
``dskip`` with ``D - 1`` eager adds, which is what a cascade step did before the sibling forms.  Algorithmic bytes of a row: the ``D`` inputs
once, the skip once, the ``D`` results once; for the backward the ``D`` cotangents, the ``D`` inputs twice, ``D`` ``dx`` and one ``dskip``."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 8.0
B = 16
# (name, C, G, H, W, Cs) and, for a resize stage, the skip's (Hs, Ws)
STAGES = [("enc_gn1", 64, 4, 120, 160, 0), ("enc_gn2", 128, 8, 60, 80, 0), ("enc_gn3", 256, 16, 30, 40, 0), ("enc_gn4", 256, 16, 15, 20, 0),
          ("enc_gn5", 512, 32, 7, 10, 0), ("enc_gn6", 1024, 64, 7, 10, 0),
          ("dec_dgn1", 512, 32, 7, 10, 512), ("dec_dgn2_plain", 256, 16, 14, 20, 0), ("dec_dgn3", 256, 16, 30, 40, 256),
          ("dec_dgn4", 128, 8, 60, 80, 128), ("dec_dgn5", 64, 4, 120, 160, 64),
          ("dec_dgn2", 256, 16, 14, 20, 256, (15, 20)), ("light_dgn2", 512, 32, 6, 10, 512, (7, 10)), ("light_dgn3", 256, 16, 14, 20, 256, (15, 20)),
          ("dec_final", 64, 4, 212, 320, 0, (213, 320))]


def eager_stage(x, w, b, G, skip, size=None):
    y = F.relu(F.group_norm(x, G, w, b, 1e-5), True)
    if size is not None:
        y = F.interpolate(y, list(size), mode="bilinear")
    if skip is None:
        return y
    return F.interpolate(torch.cat([y, skip], dim=1), scale_factor=2, mode="bilinear")


def nbytes(C, H, W, Cs, size=None):
    """-> (forward, backward) algorithmic bytes at batch B"""
    m = B * H * W * 4
    if size is not None:
        ms = B * size[0] * size[1] * 4
        if Cs == 0:      # fwd: x twice, the resized map out; bwd: gather reads g, x, writes dy; pass 2 reads dy, x, writes dx
            return 2 * C * m + C * ms, C * ms + 5 * C * m
        fwd = 2 * C * m + Cs * ms + 4 * (C + Cs) * ms
        # step 1: g -> da, dskip; gather: da, x -> dy; pass 2: dy, x -> dx
        return fwd, 4 * (C + Cs) * ms + (C + Cs) * ms + C * ms + 5 * C * m
    if Cs == 0:
        return (2 * C + C) * m, (C + C + C + C + C) * m          # bwd: pass 1 reads g, x; pass 2 reads g, x, writes dx
    fwd = (2 * C + Cs + 4 * (C + Cs)) * m
    bwd = (4 * (C + Cs) + C + C + Cs + C + C + C) * m             # pass 1: g, x -> dy, dskip; pass 2: dy, x -> dx
    return fwd, bwd


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


def main_bf16(args, sgr):
    """the same-size stages in bf16: the bf16 operator, the fp32 operator on the same values, eager under autocast on the same bf16 x"""
    reps, warm = (5, 2) if args.profile else (max(80, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "batch": B, "dtype": "bf16", "ms": {}, "bytes": {}}
    bf = torch.bfloat16
    for name, C, G, H, W, Cs, *rest in STAGES:
        if rest:
            continue      # the resize forms have no bf16 kernels ("what is left")
        g = torch.Generator().manual_seed(len(name) + C)
        x = torch.randn(B, C, H, W, generator=g).cuda().to(bf).requires_grad_(True)
        w = torch.randn(C, generator=g).cuda().requires_grad_(True)
        b = (0.3 * torch.randn(C, generator=g)).cuda().requires_grad_(True)
        skip = torch.randn(B, Cs, H, W, generator=g).cuda().to(bf).requires_grad_(True) if Cs else None
        ct = (torch.randn(B, C + Cs, 2 * H, 2 * W, generator=g) if Cs else torch.randn(B, C, H, W, generator=g)).cuda().to(bf)
        x32, ct32 = x.detach().float().requires_grad_(True), ct.float()
        skip32 = skip.detach().float().requires_grad_(True) if Cs else None
        stage = lambda x_, s_: sgr.group_norm_relu_upcat(x_, w, b, G, s_) if Cs else sgr.group_norm_relu(x_, w, b, G)

        def eager():
            with torch.autocast("cuda", dtype=bf):
                return eager_stage(x, w, b, G, skip)
        cands = dict(bf16=(lambda: stage(x, skip), [t for t in (x, w, b, skip) if t is not None], ct),
                     fp32=(lambda: stage(x32, skip32), [t for t in (x32, w, b, skip32) if t is not None], ct32),
                     eager_amp=(eager, [t for t in (x, w, b, skip) if t is not None], None))
        out_dtype = torch.float32      # autocast's group_norm, relu, cat and interpolate run in fp32 and return fp32
        if not args.profile:
            assert eager().dtype == out_dtype
        fns = {}
        for k, (f, leaves, c) in cands.items():
            if args.profile and k != "bf16":
                continue
            c = ct.to(out_dtype) if c is None else c

            def fwd(f=f):
                with torch.no_grad():
                    return f()
            fns[f"{k}_fwd"] = fwd
            fns[f"{k}_fwd_bwd"] = lambda f=f, leaves=leaves, c=c: torch.autograd.grad(f(), leaves, grad_outputs=c)
        t = timed(fns, reps, warm)
        b_fwd, b_bwd = (v // 2 for v in nbytes(C, H, W, Cs))
        rec["bytes"][name] = dict(forward=b_fwd, backward=b_bwd)
        for k, v in t.items():
            med = statistics.median(v)
            rec["ms"][f"{name}_{k}"] = dict(median=med, min=v[0], max=v[-1])
            note = ""
            if k.startswith("bf16"):
                nb = b_fwd if k == "bf16_fwd" else b_fwd + b_bwd
                floor = nb / (HBM_TBPS * 1e12) * 1e6
                note = f"algorithmic {nb / 1e6:.1f} MB (half the fp32 stage's): floor {floor:.1f} us at {HBM_TBPS} TB/s (share {floor / (med * 1e3):.2f})"
            print(f"{name + '_' + k:32s} median {med * 1e3:9.1f} us  min {v[0] * 1e3:9.1f}  max {v[-1] * 1e3:9.1f}  {note}")
        if not args.profile:
            for k in ("fwd", "fwd_bwd"):
                ours = rec["ms"][f"{name}_bf16_{k}"]
                for other in ("fp32", "eager_amp"):
                    o = rec["ms"][f"{name}_{other}_{k}"]
                    s = o["median"] / ours["median"]
                    rec["ms"][f"{name}_{other}_over_bf16_{k}"] = s
                    if s >= 1:
                        verdict = "the difference exceeds the spread" if o["min"] > ours["max"] else "THE SPREADS OVERLAP"
                    else:
                        verdict = "BF16 IS SLOWER" + ("" if ours["min"] > o["max"] else ", the spreads overlap")
                    print(f"{name + '_' + k:32s} {other} / bf16 = {s:.2f}x  ({verdict})")
        del x, w, b, skip, ct, x32, ct32, skip32, cands, fns
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


def main_siblings(args, sgr):
    """the upcat stages for D sibling decoders: one sibling call against D single calls (and autograd's D - 1 adds of dskip)"""
    D = args.siblings
    reps, warm = (5, 2) if args.profile else (max(80, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "batch": B, "siblings": D, "ms": {}, "bytes": {}}
    for name, C, G, H, W, Cs, *rest in STAGES:
        if not Cs or not name.startswith(args.only) or name.endswith("_plain"):
            continue
        Hs, Ws = rest[0] if rest else (H, W)
        g = torch.Generator().manual_seed(len(name) + C)
        xs = [torch.randn(B, C, H, W, generator=g).cuda().requires_grad_(True) for _ in range(D)]
        ws = [torch.randn(C, generator=g).cuda().requires_grad_(True) for _ in range(D)]
        bs = [(0.3 * torch.randn(C, generator=g)).cuda().requires_grad_(True) for _ in range(D)]
        skip = torch.randn(B, Cs, Hs, Ws, generator=g).cuda().requires_grad_(True)
        cts = [torch.randn(B, C + Cs, 2 * Hs, 2 * Ws, generator=g).cuda() for _ in range(D)]
        leaves = xs + ws + bs + [skip]
        one = sgr.group_norm_relu_resize_upcat if rest else sgr.group_norm_relu_upcat
        many = sgr.group_norm_relu_resize_upcat_siblings if rest else sgr.group_norm_relu_upcat_siblings
        cands = dict(siblings=lambda: list(many(xs, ws, bs, G, skip)), singles=lambda: [one(x, w, b, G, skip) for x, w, b in zip(xs, ws, bs)])
        fns = {}
        for k, f in cands.items():
            if args.profile and k != "siblings":
                continue

            def fwd(f=f):
                with torch.no_grad():
                    return f()
            fns[f"{k}_fwd"] = fwd
            fns[f"{k}_fwd_bwd"] = lambda f=f: torch.autograd.grad(f(), leaves, grad_outputs=cts)
        t = timed(fns, reps, warm)
        m, ms = B * H * W * 4, B * Hs * Ws * 4
        b_fwd = D * C * m + Cs * ms + D * 4 * (C + Cs) * ms
        b_bwd = D * 4 * (C + Cs) * ms + 2 * D * C * m + D * C * m + Cs * ms
        rec["bytes"][name] = dict(forward=b_fwd, backward=b_bwd)
        for k, v in t.items():
            med = statistics.median(v)
            rec["ms"][f"{name}_{k}"] = dict(median=med, min=v[0], max=v[-1])
            nb = b_fwd if k.endswith("_fwd") else b_fwd + b_bwd
            floor = nb / (HBM_TBPS * 1e12) * 1e6
            note = f"algorithmic {nb / 1e6:.1f} MB: floor {floor:.1f} us at {HBM_TBPS} TB/s (share {floor / (med * 1e3):.2f})"
            print(f"{name + '_' + k:32s} median {med * 1e3:9.1f} us  min {v[0] * 1e3:9.1f}  max {v[-1] * 1e3:9.1f}  {note}")
        if not args.profile:
            for k in ("fwd", "fwd_bwd"):
                sib, sin = rec["ms"][f"{name}_siblings_{k}"], rec["ms"][f"{name}_singles_{k}"]
                s = sin["median"] / sib["median"]
                rec["ms"][f"{name}_singles_over_siblings_{k}"] = s
                if s >= 1:
                    verdict = "the difference exceeds the spread" if sin["min"] > sib["max"] else "THE SPREADS OVERLAP"
                else:
                    verdict = "THE SIBLING CALL IS SLOWER" + ("" if sib["min"] > sin["max"] else ", the spreads overlap")
                print(f"{name + '_' + k:32s} D = {D}: singles / siblings = {s:.2f}x  ({verdict})")
        del xs, ws, bs, skip, cts, leaves, cands, fns
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--siblings", type=int, default=0, help="D sibling decoders: the sibling call against D single calls")
    ap.add_argument("--only", default="", help="with --siblings: the stages whose name starts with this (dec_, light_)")
    args = ap.parse_args()
    import inverserenderingofindoorscene_amd as sgr
    if not torch.cuda.is_available():
        raise SystemExit("gn_stage_bench needs a GPU")
    if args.siblings:
        return main_siblings(args, sgr)
    if args.dtype == "bf16":
        return main_bf16(args, sgr)
    reps, warm = (5, 2) if args.profile else (max(80, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "batch": B, "ms": {}, "bytes": {}}
    for name, C, G, H, W, Cs, *rest in STAGES:
        size = rest[0] if rest else None
        Hs, Ws = size if size else (H, W)
        g = torch.Generator().manual_seed(len(name) + C)
        x = torch.randn(B, C, H, W, generator=g).cuda().requires_grad_(True)
        w = torch.randn(C, generator=g).cuda().requires_grad_(True)
        b = (0.3 * torch.randn(C, generator=g)).cuda().requires_grad_(True)
        skip = torch.randn(B, Cs, Hs, Ws, generator=g).cuda().requires_grad_(True) if Cs else None
        ct = torch.randn(B, C + Cs, 2 * Hs, 2 * Ws, generator=g).cuda() if Cs else torch.randn(B, C, Hs, Ws, generator=g).cuda()
        leaves = [t for t in (x, w, b, skip) if t is not None]
        if size:
            fused = (lambda: sgr.group_norm_relu_resize_upcat(x, w, b, G, skip)) if Cs else (lambda: sgr.group_norm_relu_resize(x, w, b, G, size))
        else:
            fused = (lambda: sgr.group_norm_relu_upcat(x, w, b, G, skip)) if Cs else (lambda: sgr.group_norm_relu(x, w, b, G))
        eager = lambda: eager_stage(x, w, b, G, skip, size)

        def fwd(f):
            def run():
                with torch.no_grad():
                    return f()
            return run

        def fwdbwd(f):
            return lambda: torch.autograd.grad(f(), leaves, grad_outputs=ct)
        fns = dict(fused_fwd=fwd(fused), fused_fwd_bwd=fwdbwd(fused))
        if not args.profile:
            fns.update(eager_fwd=fwd(eager), eager_fwd_bwd=fwdbwd(eager))
        t = timed(fns, reps, warm)
        b_fwd, b_bwd = nbytes(C, H, W, Cs, size)
        rec["bytes"][name] = dict(forward=b_fwd, backward=b_bwd)
        for k, v in t.items():
            med = statistics.median(v)
            rec["ms"][f"{name}_{k}"] = dict(median=med, min=v[0], max=v[-1])
            note = ""
            if k.startswith("fused"):
                nb = b_fwd if k == "fused_fwd" else b_fwd + b_bwd
                floor = nb / (HBM_TBPS * 1e12) * 1e6
                note = f"algorithmic {nb / 1e6:.1f} MB: floor {floor:.1f} us at {HBM_TBPS} TB/s (share {floor / (med * 1e3):.2f})"
            print(f"{name + '_' + k:32s} median {med * 1e3:9.1f} us  min {v[0] * 1e3:9.1f}  max {v[-1] * 1e3:9.1f}  {note}")
        if not args.profile:
            for k in ("fwd", "fwd_bwd"):
                fu, ea = rec["ms"][f"{name}_fused_{k}"], rec["ms"][f"{name}_eager_{k}"]
                s = ea["median"] / fu["median"]
                rec["ms"][f"{name}_speedup_{k}"] = s
                if s >= 1:
                    verdict = "the difference exceeds the spread" if ea["min"] > fu["max"] else "THE SPREADS OVERLAP"
                else:
                    verdict = "FUSED IS SLOWER" + ("" if fu["min"] > ea["max"] else ", the spreads overlap")
                print(f"{name + '_' + k:32s} eager / fused = {s:.2f}x  ({verdict})")
        del x, w, b, skip, ct, leaves
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
