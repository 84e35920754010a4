"""Forward + backward time of the style variant's fused RGB layers (sivae_hip.style.to_rgb / from_rgb, csrc/rgb.hip),
plain and blended, against the eager torch chain the reference runs, on the same device in ONE process:

    python tools/bench_style_rgb.py [--iters 30] [--warmup 5] [--out profiles/style_rgb_bench.txt]

Shapes: the layer shapes of the reference's configs/ffhq256.yaml at its LOD_2_BATCH_1GPU batch sizes, K = 3.  For the
blended forms the listed shape is the feature tensor's: prev is [B, 3, H/2, W/2], the pooled image [B, 3, 2H, 2W].  Per
shape and layer the order is baseline -> new -> baseline -> new; every iteration (one forward and one backward through
torch.autograd, with gradients for every differentiable input) is timed by its own pair of HIP events after `--warmup`
untimed ones.  Reported per shape: both medians (over the two rounds), the baseline's spread (the larger of the distance
between its two rounds' medians and half of its 10 % .. 90 % range), and the bytes the fused kernels must move over the
new median (min_bytes: every tensor a direction has to read or write, once).  A shape counts as a gain only if the new
median is below the baseline's median minus the baseline's spread.  Before timing, the two implementations' outputs and
gradients are compared at the timed size.  One raw JSON line per (layer, shape) goes to --out.  Needs a ROCm device."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd"))

SHAPES = [(4, 64, 256, 256), (8, 128, 128, 128), (16, 256, 64, 64), (32, 512, 32, 32)]
K = 3
BLEND = 0.75


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "style_rgb_bench.txt"))
    args = ap.parse_args()
    import torch
    from sivae_hip import style
    if not torch.cuda.is_available():
        sys.exit("bench_style_rgb: no ROCm device (nothing is measured on the CPU)")
    F = torch.nn.functional
    dev = torch.device("cuda:0")
    lr2 = lambda t: F.leaky_relu(F.leaky_relu(t, 0.2), 0.2)  # noqa: E731
    lines = []
    for B, C, H, W in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B + C)
        r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
        leaf = lambda t: t.requires_grad_(True)  # noqa: E731
        x, prev = leaf(r(B, C, H, W)), leaf(r(B, K, H // 2, W // 2))
        wt, bt = leaf(0.1 * r(K, C, 1, 1)), leaf(0.25 * r(K))
        img, img2, other = leaf(r(B, K, H, W)), leaf(r(B, K, 2 * H, 2 * W)), leaf(r(B, C, H, W))
        wf, bf = leaf(0.5 * r(C, K, 1, 1)), leaf(0.25 * r(C))
        gk, gc = r(B, K, H, W), r(B, C, H, W)
        n, q = B * H * W, B * H * W // 4
        # name -> (leaves, upstream gradient, eager chain, fused layer, elements moved at the least)
        layers = {
            "to_rgb": ((x, wt, bt), gk, lambda: F.conv2d(x, wt, bt), lambda: style.to_rgb(x, wt, bt),
                       (C + K) * n + (K + 2 * C) * n),
            "to_rgb_blend": ((x, wt, bt, prev), gk, lambda: torch.lerp(F.interpolate(prev, size=(H, W)), F.conv2d(x, wt, bt), BLEND),
                             lambda: style.to_rgb(x, wt, bt, prev, BLEND), (C + K) * n + K * q + (K + 2 * C) * n + K * q),
            "from_rgb": ((img, wf, bf), gc, lambda: lr2(F.conv2d(img, wf, bf)), lambda: style.from_rgb(img, wf, bf),
                         (K + C) * n + (C + 2 * K) * n),
            "from_rgb_blend": ((img2, wf, bf, other), gc,
                               lambda: torch.lerp(lr2(F.conv2d(F.avg_pool2d(img2, 2, 2), wf, bf)), other, BLEND),
                               lambda: style.from_rgb(img2, wf, bf, True, other, BLEND),
                               (4 * K + 2 * C) * n + (2 * C + 8 * K) * n),
        }
        for name, (leaves, gout, base, new, elems) in layers.items():
            def step(f):
                return lambda: torch.autograd.grad(f(), leaves, gout)

            worst = 0.0
            for a, c in zip([new()] + list(step(new)()), [base()] + list(step(base)())):
                worst = max(worst, float((a.detach() - c.detach()).abs().max() / c.detach().abs().max()))
            assert worst <= 1e-3, "bench_style_rgb: %s at %s differs from the eager chain by %.2e" % (name, (B, C, H, W), worst)
            rounds = {"base": [], "new": []}
            for _ in range(2):
                rounds["base"].append(timed(torch, step(base), args.iters, args.warmup))
                rounds["new"].append(timed(torch, step(new), args.iters, args.warmup))
            allb = sorted(rounds["base"][0] + rounds["base"][1])
            med_b, med_n = statistics.median(allb), statistics.median(rounds["new"][0] + rounds["new"][1])
            spread = max(abs(statistics.median(rounds["base"][0]) - statistics.median(rounds["base"][1])),
                         0.5 * (allb[int(0.9 * (len(allb) - 1))] - allb[int(0.1 * (len(allb) - 1))]))
            nbytes = 4 * elems
            rec = dict(layer=name, shape=[B, C, H, W], base_ms=round(med_b, 4), new_ms=round(med_n, 4),
                       base_spread_ms=round(spread, 4), base_round_ms=[round(statistics.median(t), 4) for t in rounds["base"]],
                       new_round_ms=[round(statistics.median(t), 4) for t in rounds["new"]], min_bytes=nbytes,
                       new_tb_per_s=round(nbytes / (med_n * 1e-3) / 1e12, 3), gain=bool(med_n < med_b - spread),
                       max_rel_diff=worst, iters=args.iters, warmup=args.warmup)
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
