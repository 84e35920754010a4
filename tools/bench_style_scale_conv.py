"""Forward + backward time of the style variant's fused_scale convolutions (blocks._Conv3x3 with scale "up" / "down") on
the phase-form upsample-convolution kernels (functional.conv_upscale / conv_downscale) against torch's stride-2
convolutions over the four-shift kernel, the lines the blocks ran before, on the same device in ONE process:

    python tools/bench_style_scale_conv.py [--iters 20] [--warmup 3] [--layer N] [--out profiles/style_scale_conv_bench.txt]

Layers: the four fused_scale convolutions of the reference's configs/ffhq256.yaml (startf 64, maxf 512, 7 layers) at the
per-GPU batches 4 and 8.  Per layer the SAME module runs with blocks.SCALE_CONV off (base) and on (new), in the order
base -> new -> base -> new; every iteration (one forward and one backward through torch.autograd, gradients for the input
and the weight) is timed by its own pair of HIP events after `--warmup` untimed ones.  Reported per layer: mean and median
of each side over its two rounds, each round's mean, the base's spread (the larger of the distance between its two
rounds' means and half of its 10 % .. 90 % range), the routes the kernels took and the largest relative difference of
the two sides' output and gradients at the timed size.  `keep` is the rule the default follows: the layer stays on the
kernels where the new mean is not above the base mean plus the base's spread.  --layer N runs one layer (0 .. 7) and
appends to --out, so that a job can give each layer a time limit of its own.  Needs a ROCm device."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd")
sys.path[:0] = [PKG, os.path.join(PKG, "style_soft_intro_vae")]

# (network, block, kind, Ci, Co, input side)
FFHQ256 = [("generator", 5, "up", 256, 128, 64), ("generator", 6, "up", 128, 64, 128),
           ("encoder", 0, "down", 64, 128, 256), ("encoder", 1, "down", 128, 256, 128)]
LAYERS = [(B,) + l for l in FFHQ256 for B in (4, 8)]


def timed(torch, step, iters, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layer", type=int, default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "style_scale_conv_bench.txt"))
    args = ap.parse_args()
    import torch
    import blocks
    from sivae_hip import ops
    if not torch.cuda.is_available():
        sys.exit("bench_style_scale_conv: no ROCm device (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    todo = LAYERS if args.layer is None else [LAYERS[args.layer]]
    lines = []
    for B, network, block, kind, Ci, Co, side in todo:
        g = torch.Generator(device=dev).manual_seed(B + Ci + side)
        torch.manual_seed(Ci)
        m = blocks._Conv3x3(Ci, Co, kind).to(dev)
        x = torch.randn(B, Ci, side, side, generator=g, device=dev).requires_grad_(True)
        out_side = 2 * side if kind == "up" else side // 2
        gout = torch.randn(B, Co, out_side, out_side, generator=g, device=dev)
        routes = ops.scale_conv_routes(kind, B, Ci, Co, side, side)

        def run(on):
            blocks.SCALE_CONV = on
            y = m(x)
            return [y] + list(torch.autograd.grad(y, (x, m.weight), gout))

        if routes.refused:
            rec = dict(network=network, block=block, kind=kind, batch=B, channels=[Ci, Co], side=side, refused=routes.refused)
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            continue
        worst = 0.0
        for a, c in zip(run(True), run(False)):
            worst = max(worst, float((a.detach() - c.detach()).abs().max() / c.detach().abs().max()))
        assert worst <= 1e-3, "bench_style_scale_conv: %s differs from torch's convolution by %.2e" % ((B, kind, Ci, Co, side), worst)
        rounds = {"base": [], "new": []}
        for _ in range(2):
            rounds["base"].append(timed(torch, lambda: run(False), args.iters, args.warmup))
            rounds["new"].append(timed(torch, lambda: run(True), args.iters, args.warmup))
        blocks.SCALE_CONV = True
        allb, alln = sorted(rounds["base"][0] + rounds["base"][1]), rounds["new"][0] + rounds["new"][1]
        mean_b, mean_n = statistics.mean(allb), statistics.mean(alln)
        spread = max(abs(statistics.mean(rounds["base"][0]) - statistics.mean(rounds["base"][1])),
                     0.5 * (allb[int(0.9 * (len(allb) - 1))] - allb[int(0.1 * (len(allb) - 1))]))
        gflop = 3 * 2.0 * B * (2 * side if kind == "up" else side) ** 2 * Ci * Co * 9 / 1e9  # (as 3x3 convolutions, three passes)
        rec = dict(network=network, block=block, kind=kind, batch=B, channels=[Ci, Co], side=side,
                   base_ms=round(mean_b, 4), new_ms=round(mean_n, 4), base_spread_ms=round(spread, 4),
                   base_median_ms=round(statistics.median(allb), 4), new_median_ms=round(statistics.median(alln), 4),
                   base_round_ms=[round(statistics.mean(t), 4) for t in rounds["base"]],
                   new_round_ms=[round(statistics.mean(t), 4) for t in rounds["new"]],
                   keep=bool(mean_n <= mean_b + spread), new_tflops=round(gflop / mean_n, 2),
                   routes=[r.family for r in (routes.forward, routes.dgrad, routes.wgrad)],
                   max_rel_diff=worst, iters=args.iters, warmup=args.warmup)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w" if args.layer is None else "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
