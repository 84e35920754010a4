"""Forward + backward time of the style variant's fused layers (sivae_hip.style.style_layer / stat_norm, csrc/style.hip)
against an eager torch restatement of the same chain on the same device, in ONE process:

    python tools/bench_style.py [--iters 30] [--warmup 5] [--out profiles/style_bench.txt]
    python tools/bench_style.py --set blur [--out profiles/style_blur_bench.txt]

--set blur measures the chains with the blur folded in (style_layer(..., blur=True), stat_norm(..., blur=True)) against
the composition they replace (style.blur -> style_layer, stat_norm -> style.blur) with the same method and record; the two
must agree bit for bit at the timed size before anything is timed.

Shapes: the layer shapes of the reference's configs/ffhq256.yaml at its LOD_2_BATCH_1GPU batch sizes.  Per shape and
layer the order is baseline -> new -> baseline -> new; every iteration (one forward and one backward through
torch.autograd) is timed by its own pair of HIP events after `--warmup` untimed ones.  Reported per shape: both medians
(over the two rounds), the baseline's spread (the larger of the distance between its two rounds' medians and half of its
10 % .. 90 % range), and the bytes the fused kernels must move (x read and y written forward; x and dy read and dx
written backward: 5 tensors of 4 bytes an element) over the new median.  A shape counts as a gain only if the new median
is below the baseline's median minus the baseline's spread.  Before timing, the two implementations' outputs and input
gradients are compared at the timed size.  One raw JSON line per (layer, shape) goes to --out.  Needs a ROCm device."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd"))

SHAPES = [(32, 512, 32, 32), (16, 256, 64, 64), (8, 128, 128, 128), (4, 64, 256, 256)]
# --set blur: the decode / encode shapes of the same configuration from 8 x 8 up
BLUR_SHAPES = [(128, 512, 8, 8), (128, 512, 16, 16)] + SHAPES


def eager_style_layer(torch, x, nw, b, st, nz):
    F = torch.nn.functional
    t = F.leaky_relu(torch.addcmul(x, nw, nz) + b, 0.2)
    s = st.view(st.shape[0], 2, x.shape[1], 1, 1)
    return (torch.addcmul(s[:, 1], F.instance_norm(t, eps=1e-8), s[:, 0] + 1),)


def eager_stat_norm(torch, x, b):
    F = torch.nn.functional
    t = F.leaky_relu(x + b, 0.2)
    m = t.mean(dim=[2, 3], keepdim=True)
    std = torch.sqrt(((t - m) ** 2).mean(dim=[2, 3], keepdim=True))
    return F.instance_norm(t), m.flatten(1), std.flatten(1)


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


def measure(torch, name, shape, leaves, gouts, base, new, tol, nbytes, args):
    """one (layer, shape): the comparison at the timed size, then baseline -> new -> baseline -> new -> the record"""
    def step(f):
        return lambda: torch.autograd.grad(f(), leaves, gouts)

    # same results first, at the timed size: outputs and input gradients, max-norm relative
    worst = 0.0
    for a, c in zip(list(new()) + list(step(new)()), list(base()) + list(step(base)())):
        worst = max(worst, float((a.detach() - c.detach()).abs().max() / c.detach().abs().max()))
    assert worst <= tol, "bench_style: %s at %s differs from its baseline by %.2e" % (name, shape, worst)
    rounds = {"base": [], "new": []}
    for _ in range(2):
        rounds["base"].append(timed(torch, step(base), args.iters, args.warmup))
        rounds["new"].append(timed(torch, step(new), args.iters, args.warmup))
    allb = sorted(rounds["base"][0] + rounds["base"][1])
    med_b, med_n = statistics.median(allb), statistics.median(rounds["new"][0] + rounds["new"][1])
    spread = max(abs(statistics.median(rounds["base"][0]) - statistics.median(rounds["base"][1])),
                 0.5 * (allb[int(0.9 * (len(allb) - 1))] - allb[int(0.1 * (len(allb) - 1))]))
    rec = dict(layer=name, shape=list(shape), base_ms=round(med_b, 4), new_ms=round(med_n, 4),
               base_spread_ms=round(spread, 4), base_round_ms=[round(statistics.median(t), 4) for t in rounds["base"]],
               new_round_ms=[round(statistics.median(t), 4) for t in rounds["new"]], min_bytes=nbytes,
               new_tb_per_s=round(nbytes / (med_n * 1e-3) / 1e12, 3), gain=bool(med_n < med_b - spread),
               max_rel_diff=worst, iters=args.iters, warmup=args.warmup)
    print(json.dumps(rec), flush=True)
    return json.dumps(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--set", choices=("layers", "blur"), default="layers",
                    help="layers: the fused chains against eager torch; blur: the chains with the blur folded in against "
                         "the composition of the blur kernel and the chain")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join("profiles", "style_bench.txt" if args.set == "layers" else "style_blur_bench.txt")
    import torch
    from sivae_hip import style
    if not torch.cuda.is_available():
        sys.exit("bench_style: no ROCm device (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    lines = []
    for B, C, H, W in (SHAPES if args.set == "layers" else BLUR_SHAPES):
        g = torch.Generator(device=dev).manual_seed(B + C)
        r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
        x = r(B, C, H, W).requires_grad_(True)
        nw, b = (0.5 * r(1, C, 1, 1)).requires_grad_(True), (0.25 * r(1, C, 1, 1)).requires_grad_(True)
        st, nz = (0.5 * r(B, 2 * C)).requires_grad_(True), r(B, 1, H, W)
        gy, gm, gs = r(B, C, H, W), r(B, C), r(B, C)
        if args.set == "layers":
            layers = {
                "style_layer": ((x, nw, b, st), (gy,), lambda: eager_style_layer(torch, x, nw, b, st, nz),
                                lambda: (style.style_layer(x, nw, b, st, nz, True),)),
                "stat_norm": ((x, b), (gy, gm, gs), lambda: eager_stat_norm(torch, x, b), lambda: style.stat_norm(x, b)),
            }
            tol = 1e-3
        else:  # (the baseline is the composition of the project's own kernels: the fused form gives its bits)
            def norm_then_blur():
                xn, m, std = style.stat_norm(x, b)
                return style.blur(xn), m, std

            layers = {
                "blur>style_layer": ((x, nw, b, st), (gy,), lambda: (style.style_layer(style.blur(x), nw, b, st, nz, True),),
                                     lambda: (style.style_layer(x, nw, b, st, nz, True, blur=True),)),
                "stat_norm>blur": ((x, b), (gy, gm, gs), norm_then_blur, lambda: style.stat_norm(x, b, blur=True)),
            }
            tol = 0.0
        for name, (leaves, gouts, base, new) in layers.items():
            lines.append(measure(torch, name, (B, C, H, W), leaves, gouts, base, new, tol, 5 * 4 * B * C * H * W, args))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
