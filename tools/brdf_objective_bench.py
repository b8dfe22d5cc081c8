"""Times of the BRDF-stage objectives (sgr.brdf_objective, sgr.batch_ranking_loss) against an eager PyTorch restatement of the reference's
lines on the same GPU: batch 16 at 240x320 (the trainBRDF.py defaults) and at 480x640, forward and forward + backward; and the ranking
loss at B = 16, N = 800 + 800 against the per-image loop of wrapperIIW.py:88-109.

    python tools/brdf_objective_bench.py [--reps 60] [--warmup 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/brdf_objective_bench.py --profile     # the fused calls only, few repetitions

Method: device events around each call, warm-up, median of >= 60, the fused call and the eager form alternating in one process.  The
eager form keeps the reference's two ``.item()`` synchronisations (wrapperBRDF.py:118-119), and its ranking loop goes numpy -> host
tensors -> device per image as models.py:534-537 does.  The algorithmic byte counts come from the shapes: forward + backward of the full
objective reads 18 planes twice (forward, backward) and writes 8; the fused forward's second pass re-reads the 10 albedo / depth planes
on top of that (reported separately: it may come from the 256 MB Infinity Cache)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WEIGHTS = (6.0, 1.0, 0.5, 0.5)
HBM_TBPS = 8.0


def inputs(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    unit = lambda t: t / t.norm(dim=1, keepdim=True)
    aP, a = 0.05 + 0.9 * u(B, 3, H, W), u(B, 3, H, W)
    n = unit(torch.randn(B, 3, H, W, generator=g))
    nP = unit(n + 0.4 * torch.randn(B, 3, H, W, generator=g))
    r, rP = u(B, 1, H, W), 2 * u(B, 1, H, W) - 1
    d, dP = 0.5 + 4 * u(B, 1, H, W), 0.05 + 0.9 * u(B, 1, H, W)
    obj = u(B, 1, H, W) < 0.7
    seg_obj = obj.float()
    seg_all = seg_obj + (~obj & (u(B, 1, H, W) < 0.5)).float()
    return [t.cuda() for t in (aP, nP, rP, dP, a, n, r, d, seg_obj, seg_all)]


def eager_lsregress(pred, gt, origin):
    """models.py:7-21 restated"""
    nb = pred.shape[0]
    p, g = pred.reshape(nb, -1), gt.reshape(nb, -1)
    coef = torch.clamp(((p * g).sum(1) / torch.clamp((p * p).sum(1), min=1e-5)).detach(), 0.001, 1000)
    return origin * coef.reshape([nb] + [1] * (origin.dim() - 1))


def eager_objective(aP, nP, rP, dP, a, n, r, d, sB, sA, off=1.0):
    """wrapperBRDF.py:109-130 and trainBRDF.py:285 restated in eager PyTorch, the two host synchronisations included"""
    a = sB * a
    a1 = torch.clamp(eager_lsregress(aP.detach() * sB.expand_as(aP), a * sB.expand_as(a), aP), 0, 1)
    d1 = eager_lsregress(dP.detach() * sA.expand_as(dP), d * sA.expand_as(d), dP)
    n_obj = sB.sum().cpu().item()
    n_all = sA.sum().cpu().item()
    a_err = torch.sum((a1 - a) * (a1 - a) * sB.expand_as(a) / n_obj / 3.0)
    n_err = torch.sum((nP - n) * (nP - n) * sA.expand_as(n)) / n_all / 3.0
    r_err = torch.sum((rP - r) * (rP - r) * sB) / n_obj
    ld = torch.log(d1 + off) - torch.log(d + off)
    d_err = torch.sum(ld * ld * sA.expand_as(d)) / n_all
    return WEIGHTS[0] * a_err + WEIGHTS[1] * n_err + WEIGHTS[2] * r_err + WEIGHTS[3] * d_err


def rank_inputs(B, H, W, N, seed=0):
    rng = np.random.default_rng(seed)
    pt = lambda: np.concatenate([rng.integers(0, H, (B, N, 1)), rng.integers(0, W, (B, N, 1)), rng.integers(0, H, (B, N, 1)), rng.integers(0, W, (B, N, 1))], -1).astype(np.int64)
    host = dict(eqPoint=pt(), eqWeight=rng.random((B, N)).astype(np.float32), eqNum=rng.integers(N // 2, N + 1, B).astype(np.int64),
                darkerPoint=pt(), darkerWeight=rng.random((B, N)).astype(np.float32), darkerNum=rng.integers(N // 2, N + 1, B).astype(np.int64))
    albedo = (0.05 + 0.9 * torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed))).cuda()
    return albedo, host


def eager_ranking(albedo, host, tau=0.5):
    """wrapperIIW.py:88-109 with models.py:526-563 restated: a Python loop over the images, indices through the host"""
    eq_total, dk_total = 0, 0
    W = albedo.shape[3]
    for m in range(albedo.shape[0]):
        rho = torch.log(albedo[m].mean(0) + 0.001).reshape(-1)
        losses = []
        for kind in ("eq", "darker"):
            n = int(host[kind + "Num"][m])
            pt = torch.from_numpy(host[kind + "Point"][m, :n]).long().cuda()
            wt = torch.from_numpy(host[kind + "Weight"][m, :n]).float().cuda()
            f1 = torch.index_select(rho, 0, pt[:, 0] * W + pt[:, 1])
            f2 = torch.index_select(rho, 0, pt[:, 2] * W + pt[:, 3])
            losses.append(torch.mean(wt * (f1 - f2) ** 2) if kind == "eq" else torch.mean(wt * torch.relu(f2 - f1 + tau) ** 2))
        eq_total = eq_total + losses[0]
        dk_total = dk_total + losses[1]
    return eq_total / albedo.shape[0], dk_total / albedo.shape[0]


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
    q = statistics.quantiles(t, n=10)
    rec["ms"][key] = dict(median=statistics.median(t), p10=q[0], p90=q[-1])
    print(f"{key:44s} median {statistics.median(t) * 1e3:9.1f} us  p10 {q[0] * 1e3:9.1f}  p90 {q[-1] * 1e3:9.1f}  {note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import inverserenderingofindoorscene_amd as sgr
    if not torch.cuda.is_available():
        raise SystemExit("brdf_objective_bench needs a GPU")
    reps, warm = (5, 2) if args.profile else (max(60, args.reps), args.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "reps": reps, "ms": {}, "bytes": {}}
    for B, H, W in ((16, 240, 320), (16, 480, 640)):
        x = inputs(B, H, W)
        live = [t.clone().requires_grad_(True) for t in x[:4]]
        plane = B * H * W * 4
        rd_fwd, rd_b, rd_bwd, wr = 18 * plane, 10 * plane, 18 * plane, 8 * plane
        floor_us = (rd_fwd + rd_bwd + wr) / (HBM_TBPS * 1e12) * 1e6
        rec["bytes"][f"{B}x{H}x{W}"] = dict(read_forward=rd_fwd, reread_pass_b=rd_b, read_backward=rd_bwd, write_backward=wr, floor_us_at_8TBps=floor_us)

        def fused_fwd():
            with torch.no_grad():
                return sgr.brdf_objective(*x, weights=WEIGHTS).total

        def fused_fwdbwd():
            return torch.autograd.grad(sgr.brdf_objective(*live, *x[4:], weights=WEIGHTS).total, live)

        def eager_fwd():
            with torch.no_grad():
                return eager_objective(*x)

        def eager_fwdbwd():
            return torch.autograd.grad(eager_objective(*live, *x[4:]), live)

        fns = dict(fused_fwd=fused_fwd, fused_fwd_bwd=fused_fwdbwd)
        if not args.profile:
            fns.update(eager_fwd=eager_fwd, eager_fwd_bwd=eager_fwdbwd)
        t = timed(fns, reps, warm)
        tag = f"objective_B{B}_{H}x{W}_"
        for k, v in t.items():
            note = ""
            if k == "fused_fwd_bwd":
                med = statistics.median(v) * 1e3
                note = (f"algorithmic {(rd_fwd + rd_bwd + wr) / 1e6:.1f} MB (+ {rd_b / 1e6:.1f} MB re-read by pass B): floor {floor_us:.1f} us at {HBM_TBPS} TB/s, "
                        f"achieved share {floor_us / med:.2f}")
                rec["bytes"][f"{B}x{H}x{W}"]["achieved_share_of_floor"] = floor_us / med
            if k == "fused_fwd":
                note = f"floor {rd_fwd / (HBM_TBPS * 1e12) * 1e6:.1f} us for {rd_fwd / 1e6:.1f} MB (+ {rd_b / 1e6:.1f} MB re-read)"
            report(rec, tag + k, v, note)
        if not args.profile:
            for k in ("fwd", "fwd_bwd"):
                s = rec["ms"][tag + "eager_" + k]["median"] / rec["ms"][tag + "fused_" + k]["median"]
                rec["ms"][tag + "speedup_" + k] = s
                print(f"{tag + k:44s} eager / fused = {s:.1f}x")
    B, H, W, N = 16, 240, 320, 800
    albedo, host = rank_inputs(B, H, W, N)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    la = albedo.clone().requires_grad_(True)
    order = ("eqPoint", "eqWeight", "eqNum", "darkerPoint", "darkerWeight", "darkerNum")

    def rank_fused():
        eq, dk = sgr.batch_ranking_loss(la, *[dev[k] for k in order])
        return torch.autograd.grad(eq + dk, [la])

    def rank_eager():
        eq, dk = eager_ranking(la, host)
        return torch.autograd.grad(eq + dk, [la])

    fns = dict(fused_fwd_bwd=rank_fused)
    if not args.profile:
        fns["eager_fwd_bwd"] = rank_eager
    t = timed(fns, reps, warm)
    for k, v in t.items():
        report(rec, f"ranking_B{B}_N{N}_{k}", v)
    if not args.profile:
        s = rec["ms"][f"ranking_B{B}_N{N}_eager_fwd_bwd"]["median"] / rec["ms"][f"ranking_B{B}_N{N}_fused_fwd_bwd"]["median"]
        rec["ms"][f"ranking_B{B}_N{N}_speedup_fwd_bwd"] = s
        print(f"{'ranking fwd_bwd':44s} eager / fused = {s:.1f}x")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
