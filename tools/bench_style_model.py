"""Forward + backward time of the style variant's fused mapping network (sivae_hip.style.mapping), style assembly
(sivae_hip.style.styles) and model class (style_soft_intro_vae/model.py with model.FUSED) against the same tree's
per-layer / torch restatement (style.mapping_chain, torch's repeat / mean / lerp_ / where / lerp, model.FUSED = False), on
the same device in ONE process:

    python tools/bench_style_model.py [--iters 30] [--warmup 5] [--model-iters 8] [--out profiles/style_model_bench.txt]
    python tools/bench_style_model.py --count          kernel launches per generate and per model step, both settings

Legs: (i) one mapping pass, 8 layers of 512 with the pixel-norm, at B = 4, 8, 16, 32, 128, with the parameters trainable
and frozen (the E-step's and D-step's mapping_fl / mapping_tl); (ii) one styles pass at (B, 14, 512) with the running
average and with mixing; (iii) one E-step plus one D-step of the whole model (forward + backward, no optimizer) at the
configuration of the reference's configs/ffhq256.yaml, at lod 2 (16 x 16, B = 128) and lod 6 (256 x 256, B = 4).  Per
leg the order is baseline -> new -> baseline -> new; every iteration is timed by its own pair of HIP events after
`--warmup` untimed ones.  Reported per leg: both medians (over the two rounds) and the baseline's spread (the larger of
the distance between its two rounds' medians and half of its 10 % .. 90 % range).  A leg counts as a gain only if the new
median is below the baseline's median minus the baseline's spread.  One raw JSON line per leg goes to --out.  --count
runs in a process of its own (the profiler's kernel count is not taken while timing).  Needs a ROCm device."""
import argparse
import json
import os
import random
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(PKG, "style_soft_intro_vae"))

FFHQ256 = dict(startf=64, layer_count=7, maxf=512, latent_size=512, mapping_layers=8, dlatent_avg_beta=0.995,
               style_mixing_prob=0.9, channels=3, generator="GeneratorDefault", encoder="EncoderDefault", beta_kl=0.2,
               beta_rec=0.1, beta_neg=512.0, scale=0.000005)
MODEL_LEGS = [(2, 128), (6, 4)]  # (lod, batch) of LOD_2_BATCH_1GPU


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


def ab(torch, base, new, iters, warmup, **rec):
    rounds = {"base": [], "new": []}
    for _ in range(2):
        rounds["base"].append(timed(torch, base, iters, warmup))
        rounds["new"].append(timed(torch, new, iters, warmup))
    allb = sorted(rounds["base"][0] + rounds["base"][1])
    med_b, med_n = statistics.median(allb), statistics.median(rounds["new"][0] + rounds["new"][1])
    spread = max(abs(statistics.median(rounds["base"][0]) - statistics.median(rounds["base"][1])),
                 0.5 * (allb[int(0.9 * (len(allb) - 1))] - allb[int(0.1 * (len(allb) - 1))]))
    rec.update(base_ms=round(med_b, 4), new_ms=round(med_n, 4), base_spread_ms=round(spread, 4),
               base_round_ms=[round(statistics.median(t), 4) for t in rounds["base"]],
               new_round_ms=[round(statistics.median(t), 4) for t in rounds["new"]],
               gain=bool(med_n < med_b - spread), iters=iters, warmup=warmup)
    print(json.dumps(rec), flush=True)
    return json.dumps(rec)


def torch_styles(torch, s, L, s2, cutoff, avg, beta):
    """the reference's assembly (model.py:176-194) in torch"""
    styles = s.unsqueeze(1).repeat(1, L, 1)
    if beta is not None:
        with torch.no_grad():
            avg.lerp_(styles.detach().mean(dim=0), 1.0 - beta)
    if s2 is not None:
        layer = torch.arange(L, device=s.device).view(1, -1, 1)
        styles = torch.where(layer < cutoff, styles, s2.unsqueeze(1).repeat(1, L, 1))
    return styles


def model_step(torch, model_mod, m, x, lod, fused):
    def step():
        model_mod.FUSED = fused
        random.seed(0)
        for e_train in (True, False):
            for p in m.parameters():
                p.grad = None
            m(x, lod, 1, not e_train, e_train).backward()
    return step


def count_launches(torch, fn):
    """kernel launches of one call of fn, by the profiler's device-side kernel events"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None
               and "cuda" in str(e.device_type).lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model-iters", type=int, default=8)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "style_model_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_style_model: no ROCm device (nothing is measured on the CPU)")
    import model as model_mod
    from sivae_hip import style
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731

    torch.manual_seed(0)
    m = model_mod.SoftIntroVAEModelTL(**FFHQ256).to(dev)
    if args.count:
        lines = []
        for lod, B in MODEL_LEGS:
            x = r(B, 3, 4 * 2 ** lod, 4 * 2 ** lod)
            for fused in (False, True):
                def gen():
                    model_mod.FUSED = fused
                    random.seed(0)
                    with torch.no_grad():
                        m.generate(lod, 1, count=B, noise=True, no_truncation=True)
                rec = dict(leg="launches", lod=lod, B=B, fused=fused, per_generate=count_launches(torch, gen),
                           per_e_plus_d_step=count_launches(torch, model_step(torch, model_mod, m, x, lod, fused)))
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return

    lines = []
    # (i) one mapping pass
    ws = [(r(512, 512) / 512 ** 0.5).requires_grad_(True) for _ in range(8)]
    bs = [(0.1 * r(512)).requires_grad_(True) for _ in range(8)]
    for B in (4, 8, 16, 32, 128):
        x, gout = r(B, 512).requires_grad_(True), r(B, 512)
        for frozen in (False, True):
            for p in ws + bs:
                p.requires_grad_(not frozen)
            leaves = [x] + ([] if frozen else ws + bs)
            step = lambda f: (lambda: torch.autograd.grad(f(x, ws, bs, True), leaves, gout))  # noqa: E731
            a, c = style.mapping(x, ws, bs, True), style.mapping_chain(x, ws, bs, True)
            assert float((a - c).abs().max() / c.abs().max()) <= 1e-4
            lines.append(ab(torch, step(style.mapping_chain), step(style.mapping), args.iters, args.warmup,
                            leg="mapping", B=B, layers=8, width=512, frozen=frozen))
    # (ii) one styles pass
    for B in (4, 32, 128):
        s, s2, gout = r(B, 512).requires_grad_(True), r(B, 512).requires_grad_(True), r(B, 14, 512)
        avg_a, avg_b = r(14, 512), r(14, 512)
        for name, kw in (("ema", dict(s2=None, cutoff=None, beta=0.995)), ("ema_mixing", dict(s2=s2, cutoff=6, beta=0.995))):
            leaves = [s] + ([s2] if kw["s2"] is not None else [])
            base = lambda: torch.autograd.grad(torch_styles(torch, s, 14, kw["s2"], kw["cutoff"], avg_a, kw["beta"]), leaves, gout)  # noqa: E731
            new = lambda: torch.autograd.grad(style.styles(s, 14, s2=kw["s2"], cutoff=kw["cutoff"], avg=avg_b, beta=kw["beta"]), leaves, gout)  # noqa: E731
            lines.append(ab(torch, base, new, args.iters, args.warmup, leg="styles_" + name, B=B, L=14, Z=512))
    # (iii) one E-step plus one D-step of the whole model
    for lod, B in MODEL_LEGS:
        x = r(B, 3, 4 * 2 ** lod, 4 * 2 ** lod)
        lines.append(ab(torch, model_step(torch, model_mod, m, x, lod, False), model_step(torch, model_mod, m, x, lod, True),
                        args.model_iters, 2, leg="model_e_plus_d", lod=lod, B=B, res=4 * 2 ** lod))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
