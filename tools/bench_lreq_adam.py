"""Time of the style variant's optimizer work in one iteration of the introspective phase (encoder step + decoder step +
weight average) with sivae_hip.lreq_adam (multi-tensor HIP launches, csrc/multi_tensor.hip) against an eager restatement
of what the reference does (five element-wise torch ops per tensor and one lerp_ per tensor), on the same device in ONE
process:

    python tools/bench_lreq_adam.py [--iters 30] [--warmup 5] [--out profiles/lreq_adam_bench.txt]

Parameters: the tensors of the reference's configs/ffhq256.yaml model (startf 64, maxf 512, 7 layers, latent 512, 8 mapping
layers, its default encoder), shapes and lr_equalization_coef from the constructors of style_soft_intro_vae/blocks.py
(built on the meta device) and, for what blocks.py does not cover (from_rgb, to_rgb, const, the mapping networks), by
formula; the counts are checked: decoder + mapping_fl 100 tensors / 26.1 M elements, encoder + mapping_tl 76 tensors /
27.8 M.  Gradients are random and every tensor has one.

The order is baseline -> new -> baseline -> new, `--iters` iterations each after `--warmup` untimed ones.  The gain is on
the host side, so two clocks are reported: HIP events around every iteration (and around its two steps alone), and the
wall-clock time of the whole synchronised batch of iterations divided by their number.  Medians over the two rounds; the
baseline's spread is the larger of the distance between its two rounds' medians and half of its 10 % .. 90 % range; a
gain counts only if the new median is below the baseline's median minus that spread.  Launches per iteration: from
`last_step` (new) and counted by the eager loop (baseline).  The fused steps read p, g, v and write p, v: 20 bytes an
element, set against 6.3 TB/s.  Before timing, one iteration of each is compared.  Raw JSON goes to --out.  Needs a ROCm
device."""
import argparse
import json
import math
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(PKG, "style_soft_intro_vae"))

STARTF, MAXF, LAYERS, LATENT, MAPPING_LAYERS, CHANNELS = 64, 512, 7, 512, 8, 3
HBM_TB_PER_S = 6.3


def _linear(specs, i, o, gain=math.sqrt(2.0), lrmul=1.0):
    specs += [((o, i), gain / math.sqrt(i) * lrmul), ((o,), lrmul)]


def _block(specs, block):
    specs += [(tuple(p.shape), getattr(p, "lr_equalization_coef", None)) for p in block.parameters()]


def model_specs(torch):
    """-> {"decoder": [(shape, coef or None)], "encoder": [...]}: decoder + mapping_fl and encoder + mapping_tl"""
    import blocks
    dec, enc = [], []
    with torch.device("meta"):
        mul = 2 ** (LAYERS - 1)
        inputs = min(MAXF, STARTF * mul)
        dec.append(((1, inputs, 4, 4), None))  # const
        res = 2
        for i in range(LAYERS):
            outputs = min(MAXF, STARTF * mul)
            _block(dec, blocks.DecodeBlock(inputs, outputs, LATENT, i != 0, fused_scale=res * 2 >= 128, layer=i))
            dec += [((CHANNELS, outputs, 1, 1), 0.03 / math.sqrt(outputs)), ((CHANNELS,), 1.0)]  # to_rgb
            res, inputs, mul = res * 2, outputs, mul // 2
        for i in range(MAPPING_LAYERS):  # mapping_fl
            _linear(dec, LATENT, LATENT, lrmul=0.1)
        mul, inputs, res = 2, STARTF, 2 ** (LAYERS + 1)
        for i in range(LAYERS):
            outputs = min(MAXF, STARTF * mul)
            enc += [((inputs, CHANNELS, 1, 1), math.sqrt(2.0) / math.sqrt(CHANNELS)), ((inputs,), 1.0)]  # from_rgb
            _block(enc, blocks.EncodeBlock(inputs, outputs, LATENT, False, fused_scale=res >= 128))
            res, inputs, mul = res // 2, outputs, mul * 2
        for i in range(3):  # mapping_tl: the last layer gives mean and log-variance
            _linear(enc, LATENT, 2 * LATENT if i == 2 else LATENT, lrmul=0.1)
    return {"decoder": dec, "encoder": enc}


def make_params(torch, specs, dev, gen):
    ps = []
    for shape, coef in specs:
        p = torch.nn.Parameter(torch.randn(*shape, device=dev, generator=gen))
        p.grad = torch.randn(*shape, device=dev, generator=gen) * 10.0 ** float(torch.rand((), generator=gen, device=dev) * 4 - 3)
        if coef is not None:
            p.lr_equalization_coef = coef
        ps.append(p)
    return ps


class EagerLREQAdam:
    """the reference's loop: mul_, addcmul_, sqrt, add_, addcdiv_ per tensor"""

    def __init__(self, params, lr, beta_2=0.99, eps=1e-8):
        self.params, self.lr, self.beta_2, self.eps, self.state, self.launches = params, lr, beta_2, eps, {}, 0

    def step(self):
        self.launches = 0
        for p in self.params:
            if p.grad is None:
                continue
            st = self.state.setdefault(p, {"step": 0, "exp_avg_sq": p.data.new_zeros(p.shape)})
            st["step"] += 1
            v, g = st["exp_avg_sq"], p.grad.data
            v.mul_(self.beta_2).addcmul_(g, g, value=1 - self.beta_2)
            denom = v.sqrt().add_(self.eps)
            p.data.addcdiv_(g, denom, value=-self.lr * math.sqrt(1 - self.beta_2 ** st["step"])
                            * getattr(p, "lr_equalization_coef", 1.0))
            self.launches += 5


def timed(torch, iteration, iters, warmup):
    """-> (per-iteration event ms, per-iteration event ms of the two steps alone, wall ms per iteration of the batch)"""
    for _ in range(warmup):
        iteration(None)
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    t0 = time.perf_counter()
    for a, b, c in evs:
        a.record()
        iteration(b)
        c.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    return [a.elapsed_time(c) for a, b, c in evs], [a.elapsed_time(b) for a, b, c in evs], wall


def spread_of(rounds):
    allv = sorted(rounds[0] + rounds[1])
    return max(abs(statistics.median(rounds[0]) - statistics.median(rounds[1])),
               0.5 * (allv[int(0.9 * (len(allv) - 1))] - allv[int(0.1 * (len(allv) - 1))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "lreq_adam_bench.txt"))
    args = ap.parse_args()
    import torch
    from sivae_hip.lreq_adam import LREQAdam, lerp_parameters
    if not torch.cuda.is_available():
        sys.exit("bench_lreq_adam: no ROCm device (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    specs = model_specs(torch)
    counts = {k: (len(v), sum(math.prod(s) for s, _ in v)) for k, v in specs.items()}
    assert counts["decoder"][0] == 100 and abs(counts["decoder"][1] / 1e6 - 26.1) < 0.05, counts
    assert counts["encoder"][0] == 76 and abs(counts["encoder"][1] / 1e6 - 27.8) < 0.05, counts
    elements = counts["decoder"][1] + counts["encoder"][1]
    weight = 1.0 - 0.5 ** (32 / (10 * 1000.0))

    def side(seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        nets = {k: make_params(torch, v, dev, gen) for k, v in specs.items()}
        avg = [torch.randn(p.shape, device=dev, generator=gen) for k in ("encoder", "decoder") for p in nets[k]]  # the averaged model's tensors
        return nets, avg

    (new_nets, new_avg), (base_nets, base_avg) = side(1), side(1)
    new_opts = [LREQAdam(new_nets[k], lr=1.5e-3) for k in ("encoder", "decoder")]
    base_opts = [EagerLREQAdam(base_nets[k], lr=1.5e-3) for k in ("encoder", "decoder")]
    new_all, base_all = new_nets["encoder"] + new_nets["decoder"], base_nets["encoder"] + base_nets["decoder"]
    launches = {}

    def new_iteration(mid):
        for o in new_opts:
            o.step()
        if mid is not None:
            mid.record()
        r = lerp_parameters(new_avg, new_all, weight)
        launches["new"] = sum(o.last_step["launches"] for o in new_opts) + r["launches"]
        assert r["fallback"] == 0 and all(o.last_step["fallback"] == 0 for o in new_opts)

    def base_iteration(mid):
        for o in base_opts:
            o.step()
        if mid is not None:
            mid.record()
        for p, q in zip(base_avg, base_all):
            p.data.lerp_(q.data, weight)
        launches["base"] = sum(o.launches for o in base_opts) + len(base_avg)

    # the same results first: one iteration of each from the same state
    new_iteration(None)
    base_iteration(None)
    worst = max(float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
                for xs, ys in ((new_all, base_all), (new_avg, base_avg)) for a, b in zip(xs, ys))
    assert worst <= 1e-5, "bench_lreq_adam: the fused iteration differs from the eager one by %.2e" % worst

    rounds = {k: {"event": [], "steps": [], "wall": []} for k in ("base", "new")}
    for _ in range(2):
        for k, it in (("base", base_iteration), ("new", new_iteration)):
            ev, st, wall = timed(torch, it, args.iters, args.warmup)
            rounds[k]["event"].append(ev)
            rounds[k]["steps"].append(st)
            rounds[k]["wall"].append(wall)
    med = {k: {c: statistics.median(v[c][0] + v[c][1]) for c in ("event", "steps")} for k, v in rounds.items()}
    spread = spread_of(rounds["base"]["event"])
    wall = {k: statistics.mean(v["wall"]) for k, v in rounds.items()}
    wall_spread = abs(rounds["base"]["wall"][0] - rounds["base"]["wall"][1])
    step_bytes = 20 * elements
    roof_ms = step_bytes / (HBM_TB_PER_S * 1e12) * 1e3
    rec = dict(tensors={k: v[0] for k, v in counts.items()}, elements={k: v[1] for k, v in counts.items()},
               base_event_ms=round(med["base"]["event"], 4), new_event_ms=round(med["new"]["event"], 4),
               base_event_spread_ms=round(spread, 4), gain_event=bool(med["new"]["event"] < med["base"]["event"] - spread),
               base_event_round_ms=[round(statistics.median(t), 4) for t in rounds["base"]["event"]],
               new_event_round_ms=[round(statistics.median(t), 4) for t in rounds["new"]["event"]],
               base_wall_ms=round(wall["base"], 4), new_wall_ms=round(wall["new"], 4),
               base_wall_round_ms=[round(t, 4) for t in rounds["base"]["wall"]],
               new_wall_round_ms=[round(t, 4) for t in rounds["new"]["wall"]], base_wall_spread_ms=round(wall_spread, 4),
               gain_wall=bool(wall["new"] < wall["base"] - wall_spread),
               base_steps_event_ms=round(med["base"]["steps"], 4), new_steps_event_ms=round(med["new"]["steps"], 4),
               launches_per_iteration=dict(launches), step_bytes=step_bytes, roofline_ms=round(roof_ms, 4),
               new_steps_over_roofline=round(med["new"]["steps"] / roof_ms, 2),
               new_steps_tb_per_s=round(step_bytes / (med["new"]["steps"] * 1e-3) / 1e12, 3),
               max_rel_diff=worst, iters=args.iters, warmup=args.warmup)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
