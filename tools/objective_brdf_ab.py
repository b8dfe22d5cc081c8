"""The light objective with BRDF-map gradients at config 2 (16 images, 240x320 -> 120x160, 12 lobes, 8x16 directions), five variants
alternating in one process, each step timed with device events after a warm-up:

  (a) light_objective, SG parameters live (the default route), forward + backward
  (b) light_objective(..., brdf_grads=True), normal and rough live as well (wrapperBRDFLight.py:194 detaches albedoPred only)
  (c) light_objective(..., brdf_grads=True), all three maps live
  (d) forwardSG(need_env=True) + render_loss + recon_loss + backward, normal and rough live (what such a caller ran before brdf_grads)
  (e) (a) followed by the layer's BRDF backward from the SG lobes composed by hand (sgrender::render_bwd_brdf with env = None, random
      render cotangents): what (b) does inside one operator, as a cross-check of its cost

Usage: python tools/objective_brdf_ab.py [--steps N] [--warmup W] [--rounds R] [--out FILE]
Prints one line per variant (median / p10 / p90 / min in ms) and the ratios, and writes them as JSON to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the variants")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import inverserenderingofindoorscene_amd as sgr
    from oracle import sg_oracle as O

    bn, imH, imW, R, C, K = 16, 240, 320, 120, 160, 12
    inp = {k: v.cuda() for k, v in O.synthetic_inputs(bn, imH, imW, R, C, K, seed=2024).items()}
    ind = torch.ones(bn, 1, 1, 1, device="cuda")
    layer = sgr.renderingLayer(imWidth=C, imHeight=R)
    SG, MAPS = ("axis", "lamb", "weight"), ("albedo", "normal", "rough")

    def leaves(live):
        return {k: (v.detach().requires_grad_(True) if k in live else v) for k, v in inp.items()}

    def fused(live, brdf):
        x = leaves(live)
        ins = [x[k] for k in SG + MAPS if k in live]

        def step():
            obj = sgr.light_objective(layer, x["albedo"], x["normal"], x["rough"], x["axis"], x["lamb"], x["weight"], x["im"], x["seg"], x["env_gt"],
                                      ind, 1.0, 10.0, brdf_grads=brdf)
            return torch.autograd.grad(obj[0], ins)
        return step

    def unfused(live):
        x = leaves(live)
        ins = [x[k] for k in SG + MAPS if k in live]

        def step():
            env, d, s = layer.forwardSG(x["albedo"], x["normal"], x["rough"], x["axis"], x["lamb"], x["weight"], need_env=True)
            err, _ = sgr.render_loss(d, s, x["im"], x["seg"], R, C)
            rec = sgr.recon_loss(env, x["env_gt"], x["seg"], ind, R, C)
            return torch.autograd.grad(err + 10.0 * rec, ins)
        return step

    def separate():
        f = fused(SG, False)
        gd, gs = torch.randn(bn, 3, R, C, device="cuda"), torch.randn(bn, 3, R, C, device="cuda")

        def step():
            g = f()
            return g + sgr.ops.ops.render_bwd_brdf(gd, gs, inp["albedo"], inp["normal"], inp["rough"], None, inp["axis"], inp["lamb"], inp["weight"],
                                                   8, 16, layer.fov_deg, float(layer.F0), [0.0, 0.0, 0.0], True)
        return step

    variants = {
        "a_sg_only": fused(SG, False),
        "b_brdf_normal_rough": fused(SG + ("normal", "rough"), True),
        "c_brdf_all_maps": fused(SG + MAPS, True),
        "d_unfused_normal_rough": unfused(SG + ("normal", "rough")),
        "e_separate_pass": separate(),
    }
    times = {k: [] for k in variants}
    for k, f in variants.items():
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for _ in range(args.rounds):
        for k, f in variants.items():
            for _ in range(3):
                f()
            for e0, e1 in ev:
                e0.record()
                f()
                e1.record()
            torch.cuda.synchronize()
            times[k] += [e0.elapsed_time(e1) for e0, e1 in ev]
    rec = {"config": dict(bn=bn, imH=imH, imW=imW, R=R, C=C, K=K, eh=8, ew=16), "steps_per_variant": args.steps * args.rounds,
           "device": torch.cuda.get_device_name(0), "ms": {}}
    for k, t in times.items():
        t = sorted(t)
        q = statistics.quantiles(t, n=10)
        rec["ms"][k] = dict(median=statistics.median(t), p10=q[0], p90=q[-1], min=t[0])
        print(f"{k:24s} median {statistics.median(t):.4f} ms  p10 {q[0]:.4f}  p90 {q[-1]:.4f}  min {t[0]:.4f}")
    md = {k: v["median"] for k, v in rec["ms"].items()}
    rec["b_over_d"] = md["b_brdf_normal_rough"] / md["d_unfused_normal_rough"]
    rec["b_minus_a_us"] = 1e3 * (md["b_brdf_normal_rough"] - md["a_sg_only"])
    rec["c_minus_a_us"] = 1e3 * (md["c_brdf_all_maps"] - md["a_sg_only"])
    rec["e_minus_a_us"] = 1e3 * (md["e_separate_pass"] - md["a_sg_only"])
    print(f"(b)/(d) = {rec['b_over_d']:.3f}   (b)-(a) = {rec['b_minus_a_us']:.1f} us   (c)-(a) = {rec['c_minus_a_us']:.1f} us   (e)-(a) = {rec['e_minus_a_us']:.1f} us")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
